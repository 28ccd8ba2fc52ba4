"""Host-side mirror of the reference's ``mlmap`` class (include/mlmap.h:42-140) over the C ABI of
``include/mlmap_hip.h``.

Only the map-update path and its queries are mirrored: ``update_map``, ``getOccupancy``, ``getOdd``,
``getOddGrad``, ``setFree_map_in_bound`` (+ ``getInflateOccupancy``, ``inflate_map``).  ROS plumbing
(subscriptions, TF, RViz) is out of scope.

This module is pure plumbing: ctypes calls into ``libmlmap_hip.so``.  There is no CPU fallback — if the
library is missing or no MI355X is visible, construction raises.
"""
from __future__ import annotations

import ctypes
import importlib.util
import math
import os
import sys
from typing import Dict, List, Optional, Tuple

import numpy as np

from .config import CConfig, MapConfig, to_c

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MLMAP_HIP_LIB") or os.path.join(_HERE, "lib", "libmlmap_hip.so")  # env: development builds

MLM_OK = 0
# mlm_export_esdf flags (include/mlmap_hip.h): obstacle predicates (their union) and the signed field
MLM_ESDF_OCC, MLM_ESDF_INFL, MLM_ESDF_UNKNOWN, MLM_ESDF_SIGNED = 1, 2, 4, 8
# mlm_export_grid2d: the class bits (their union), "unobserved cells are obstacles of the distance too", int32 per column row
MLM_GRID_OCC, MLM_GRID_INFL, MLM_GRID_UNKNOWN, MLM_GRID_DIST_UNOBSERVED, MLM_GRID_COL = 1, 2, 4, 16, 8
# mlm_export_reach: obstacle predicates (their union; none: no obstacles), steps of a voxel not reached, parent code of a seed
MLM_REACH_OCC, MLM_REACH_INFL, MLM_REACH_UNKNOWN, MLM_REACH_NONE, MLM_REACH_SEED = 1, 2, 4, -1, 6
# mlm_export_route: the same predicates, cost of a voxel not reached, parent code of a seed (0..25 are the moves' codes)
MLM_ROUTE_OCC, MLM_ROUTE_INFL, MLM_ROUTE_UNKNOWN, MLM_ROUTE_NONE, MLM_ROUTE_SEED = 1, 2, 4, -1, 26
MLM_PATH_REACH, MLM_PATH_ROUTE, MLM_PATH_ROW = 0, 1, 8
MLM_SCORE_CLASSES, MLM_SCORE_ROW = 1, 8
# mlm_query_clearance: the flag, min_sq of a ray that saw no voxel, the status of a walk that left the box, int64 per group row
MLM_CLEAR_OUTSIDE_PASS, MLM_CLEAR_NONE, MLM_CLEAR_LEFT, MLM_CLEAR_ROW = 1, -1, 2, 8
# mlm_export_clusters: the set (FRONTIER alone, or a union of the class bits), labels off the set / in a dropped component, int64 per row
MLM_CLUSTER_OCC, MLM_CLUSTER_INFL, MLM_CLUSTER_UNKNOWN, MLM_CLUSTER_FRONTIER = 1, 2, 4, 16
MLM_CLUSTER_NONE, MLM_CLUSTER_SMALL, MLM_CLUSTER_ROW = -1, -2, 16
# mlm_export_mesh: the class bits (their union), faces towards FREE voxels only, the box closed against its outside, int64 in summary
MLM_MESH_OCC, MLM_MESH_INFL, MLM_MESH_UNKNOWN, MLM_MESH_SEEN, MLM_MESH_CLOSED, MLM_MESH_ROW = 1, 2, 4, 16, 32, 12
# mlm_export_octree: infl == OCCUPIED counts as OCC, FREE voxels count as NONE, int64 in summary; the labels a word holds per child
MLM_OCT_INFL, MLM_OCT_OCC_ONLY, MLM_OCT_ROW = 1, 2, 40
MLM_OCT_NONE, MLM_OCT_FREE, MLM_OCT_OCC, MLM_OCT_INNER = 0, 1, 2, 3
# mlm_crop_blocks flags (OUTSIDE / INSIDE: which side of the key box is dropped), int64 in summary
MLM_CROP_OUTSIDE, MLM_CROP_INSIDE, MLM_CROP_DRY, MLM_CROP_SHRINK, MLM_CROP_ROW = 0, 1, 2, 4, 8
# mlm_warp_blocks flags, int64 in summary
MLM_WARP_SEEN, MLM_WARP_REPLACE, MLM_WARP_DRY, MLM_WARP_ROW = 1, 2, 4, 8
# mlm_fuse_blocks modes and flag, int64 in summary, int32 per row of per_row
MLM_FUSE_ADD, MLM_FUSE_MAX, MLM_FUSE_TAKE, MLM_FUSE_FILL, MLM_FUSE_DRY, MLM_FUSE_ROW, MLM_FUSE_COLS = 0, 1, 2, 3, 1, 12, 4
FUSE_MODES = {"add": MLM_FUSE_ADD, "max": MLM_FUSE_MAX, "take": MLM_FUSE_TAKE, "fill": MLM_FUSE_FILL}
# mlm_age_blocks modes and flags, int64 in summary, int32 per block of per_block
MLM_AGE_SCALE, MLM_AGE_STEP, MLM_AGE_ROW, MLM_AGE_COLS = 0, 1, 12, 4
MLM_AGE_OUTSIDE, MLM_AGE_DRY, MLM_AGE_FORGET, MLM_AGE_DROP, MLM_AGE_CLEAR_INFL = 1, 2, 4, 8, 16
AGE_MODES = {"scale": MLM_AGE_SCALE, "step": MLM_AGE_STEP}
# mlm_delta_blocks flags, int64 in summary, the values of its kind output
MLM_DELTA_DRY, MLM_DELTA_NO_INFL, MLM_DELTA_ROW = 1, 2, 12
MLM_DELTA_CHANGED, MLM_DELTA_NEW = 1, 2
# mlm_pack_blocks flags, int64 in the summary of mlm_pack_blocks and mlm_unpack_blocks
MLM_PACK_DRY, MLM_PACK_NO_INFL, MLM_PACK_ROW = 1, 2, 8
# mlm_query_rays flags: what stops a ray (their union; 0: nothing, a pure count)
MLM_RAY_OCC, MLM_RAY_INFL, MLM_RAY_UNKNOWN = 1, 2, 4
# mlm_query_views: int64 per row of the table
MLM_VIEW_ROW = 8
# mlm_render_depth: int64 per row of the table
MLM_RENDER_ROW = 4
# mlm_query_boxes flags: what blocks a box (their union; 0: nothing), int64 per row of the table
MLM_BOX_OCC, MLM_BOX_INFL, MLM_BOX_UNKNOWN, MLM_BOX_ROW = 1, 2, 4, 4
STATUS = {0: "MLM_OK", -1: "MLM_ERR_INVALID", -2: "MLM_ERR_HIP", -3: "MLM_ERR_CAPACITY", -4: "MLM_ERR_UNSUPPORTED"}

# every symbol include/mlmap_hip.h declares
ABI_SYMBOLS = [
    "mlm_create", "mlm_destroy", "mlm_last_error", "mlm_abi_version", "mlm_set_stream",
    "mlm_integrate_depth_u16", "mlm_integrate_depth_u16_dev", "mlm_integrate_depth_batch_dev",
    "mlm_integrate_depth_batch", "mlm_integrate_callback",
    "mlm_integrate_points", "mlm_query_occupancy", "mlm_query_occupancy_inflate", "mlm_query_inflate_occupancy",
    "mlm_query_odds", "mlm_query_odd_grad", "mlm_query_odds_at", "mlm_export_frontier_points", "mlm_import_blocks", "mlm_crop_blocks", "mlm_warp_blocks", "mlm_fuse_blocks", "mlm_age_blocks", "mlm_delta_blocks",
    "mlm_pack_blocks", "mlm_unpack_blocks", "mlm_merge_pack", "mlm_merge_finish",
    "mlm_set_free_in_bound", "mlm_inflate_map", "mlm_block_count",
    "mlm_export_blocks", "mlm_export_block_flags", "mlm_export_window", "mlm_export_esdf", "mlm_export_grid2d", "mlm_export_reach", "mlm_export_route", "mlm_export_clusters", "mlm_export_mesh", "mlm_export_octree", "mlm_query_rays", "mlm_render_depth", "mlm_query_views", "mlm_query_boxes", "mlm_query_nearest", "mlm_query_sweeps", "mlm_query_paths", "mlm_score_poses", "mlm_query_clearance", "mlm_export_frontier", "mlm_export_global_map", "mlm_sync", "mlm_set_async", "mlm_set_host_mirror_limit", "mlm_get_frame_stats",
    "mlm_get_awareness_hits",
    "mlm_get_awareness_misses", "mlm_get_T_ls", "mlm_get_odds_table", "mlm_get_kernel_times",
    "mlm_enable_kernel_timing", "mlm_set_timed_kernel", "mlm_host_register", "mlm_host_unregister", "mlm_debug_set", "mlm_debug_reset",
    "mlm_debug_clocks", "mlm_debug_probe_seeds",
]


class MlmError(RuntimeError):
    pass


class Limits(ctypes.Structure):
    _fields_ = [("max_blocks", ctypes.c_int32), ("max_points", ctypes.c_int32), ("max_batch", ctypes.c_int32),
                ("record_awareness", ctypes.c_int32)]


class FrameStats(ctypes.Structure):
    _fields_ = [("n_points", ctypes.c_int64), ("n_hit_cells", ctypes.c_int64), ("n_miss_cells", ctypes.c_int64),
                ("n_out_of_range", ctypes.c_int64), ("n_blocks", ctypes.c_int64), ("n_rehash_epochs", ctypes.c_int64),
                ("hit_bucket_count", ctypes.c_int64), ("n_multi_cells", ctypes.c_int64),
                ("n_contrib_slots", ctypes.c_int64), ("n_groups", ctypes.c_int64), ("n_rays", ctypes.c_int64),
                ("n_spec_replays", ctypes.c_int64), ("n_device_atomics", ctypes.c_int64), ("n_sector_fallbacks", ctypes.c_int64),
                ("logit_bit_exact", ctypes.c_int64), ("n_pool_grows", ctypes.c_int64), ("block_capacity", ctypes.c_int64),
                ("n_graph_launches", ctypes.c_int64), ("n_bin_exact_waves", ctypes.c_int64),
                ("n_host_queries", ctypes.c_int64), ("n_mirror_refreshes", ctypes.c_int64), ("n_mirror_blocks", ctypes.c_int64),
                ("device_bytes", ctypes.c_int64), ("n_slot_grows", ctypes.c_int64)]

    def as_dict(self) -> Dict[str, int]:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


_lib = None


def _share_hip_runtime_with_torch():
    """A process can drive the GPU through ONE HIP/HSA runtime only.  libmlmap_hip.so asks for `libamdhip64.so.7`
    (the system ROCm); PyTorch-ROCm wheels bundle their own copy and ask for it by another name, so importing torch
    AFTER this library would bring a second runtime that finds "no ROCm-capable device".  When a torch installation is
    present (it owns streams / RCCL in bench.py and in the merge), load ITS runtime first: the library then binds to it
    through the shared soname, whichever of the two is imported first.  MLMAP_HIP_RUNTIME=system keeps the system one
    (hosts without torch, e.g. the C++ facade, are not affected either way)."""
    if "torch" in sys.modules or os.environ.get("MLMAP_HIP_RUNTIME") == "system":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)


def load_library(path: Optional[str] = None):
    """dlopen libmlmap_hip.so and declare the prototypes.  Raises if the library is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise MlmError(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    _share_hip_runtime_with_torch()
    L = ctypes.CDLL(p)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.mlm_create.argtypes = [vp, vp, i32, ctypes.POINTER(vp)]
    L.mlm_destroy.argtypes = [vp]
    L.mlm_last_error.argtypes = [vp]
    L.mlm_last_error.restype = ctypes.c_char_p
    L.mlm_set_stream.argtypes = [vp, vp]
    L.mlm_integrate_depth_u16.argtypes = [vp, vp, i32, i32, i32, vp, i32, vp, vp]
    L.mlm_integrate_depth_u16_dev.argtypes = [vp, vp, i32, i32, i32, vp, i32, vp, vp]
    L.mlm_integrate_depth_batch_dev.argtypes = [vp, vp, i32, ctypes.c_size_t, i32, i32, i32, vp, vp]
    L.mlm_integrate_depth_batch.argtypes = [vp, vp, i32, ctypes.c_size_t, i32, i32, i32, vp, vp]
    L.mlm_integrate_points.argtypes = [vp, vp, i32, vp, vp]
    L.mlm_integrate_callback.argtypes = [vp, vp, i32, i32, i32, ctypes.c_double, vp, vp, vp, ctypes.c_double, vp,
                                         ctypes.c_double, ctypes.c_double, i32, vp]
    L.mlm_query_occupancy.argtypes = [vp, vp, i32, vp]
    L.mlm_query_occupancy_inflate.argtypes = [vp, vp, i32, ctypes.c_float, vp]
    L.mlm_query_inflate_occupancy.argtypes = [vp, vp, i32, vp]
    L.mlm_query_odds.argtypes = [vp, vp, i32, vp]
    L.mlm_query_odd_grad.argtypes = [vp, vp, i32, i32, vp]
    L.mlm_query_odds_at.argtypes = [vp, vp, vp, i32, vp]
    L.mlm_export_frontier_points.argtypes = [vp, i32, vp, vp]
    L.mlm_import_blocks.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.mlm_crop_blocks.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.mlm_warp_blocks.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp]
    L.mlm_fuse_blocks.argtypes = [vp, i32, vp, vp, vp, vp, i32, i32, vp, vp]
    L.mlm_age_blocks.argtypes = [vp, vp, vp, i32, ctypes.c_float, ctypes.c_float, i32, vp, vp]
    L.mlm_delta_blocks.argtypes = [vp, vp, vp, i32, vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp]
    L.mlm_pack_blocks.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, i32, ctypes.c_size_t, vp, vp]
    L.mlm_unpack_blocks.argtypes = [vp, vp, ctypes.c_size_t, i32, i32, vp, vp, vp, vp, vp]
    L.mlm_merge_pack.argtypes = [vp, vp, i32, vp, vp]
    L.mlm_merge_finish.argtypes = [vp, vp, vp, ctypes.c_size_t, vp]
    L.mlm_set_free_in_bound.argtypes = [vp, vp, vp]
    L.mlm_inflate_map.argtypes = [vp, vp]
    L.mlm_block_count.argtypes = [vp, vp]
    L.mlm_export_blocks.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.mlm_export_window.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp]
    L.mlm_export_esdf.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp]
    L.mlm_export_grid2d.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    L.mlm_export_reach.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp]
    L.mlm_export_route.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, i32, i32, vp, vp, vp]
    L.mlm_export_clusters.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, i32, vp]
    L.mlm_export_mesh.argtypes = [vp, vp, vp, i32, vp, vp, ctypes.c_int64, vp, vp, vp, ctypes.c_int64, vp]
    L.mlm_export_octree.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, ctypes.c_int64, vp, vp, ctypes.c_int64, vp]
    L.mlm_query_rays.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp]
    L.mlm_render_depth.argtypes = [vp, vp, i32, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp]
    L.mlm_query_views.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp]
    L.mlm_query_boxes.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.mlm_query_nearest.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]
    L.mlm_query_sweeps.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.mlm_query_paths.argtypes = [vp, vp, vp, vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp]
    L.mlm_score_poses.argtypes = [vp, vp, i32, vp, i32, i32, vp, vp, vp, i32, vp]
    L.mlm_query_clearance.argtypes = [vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp]
    L.mlm_export_global_map.argtypes = [vp, i32, vp, vp]
    L.mlm_export_block_flags.argtypes = [vp, i32, vp, vp]
    L.mlm_export_frontier.argtypes = [vp, i32, vp, vp]
    L.mlm_sync.argtypes = [vp]
    L.mlm_set_async.argtypes = [vp, i32]
    L.mlm_set_host_mirror_limit.argtypes = [vp, ctypes.c_size_t]
    L.mlm_get_frame_stats.argtypes = [vp, vp]
    L.mlm_get_awareness_hits.argtypes = [vp, i32, vp, vp, vp, vp]
    L.mlm_get_awareness_misses.argtypes = [vp, i32, vp, vp]
    L.mlm_get_T_ls.argtypes = [vp, vp, vp]
    L.mlm_get_odds_table.argtypes = [vp, vp]
    L.mlm_get_kernel_times.argtypes = [vp, i32, vp, vp, vp]
    L.mlm_enable_kernel_timing.argtypes = [vp, i32]
    L.mlm_set_timed_kernel.argtypes = [vp, ctypes.c_char_p, i32]
    L.mlm_host_register.argtypes = [vp, vp, ctypes.c_size_t]
    L.mlm_host_unregister.argtypes = [vp, vp]
    L.mlm_debug_set.argtypes = [ctypes.c_char_p, ctypes.c_longlong]
    L.mlm_debug_reset.argtypes = []
    L.mlm_debug_clocks.argtypes = [vp, vp, i32]
    L.mlm_debug_probe_seeds.argtypes = [vp, vp]
    if path is None and os.environ.get("MLM_KNOBS"):
        # tooling convenience (tools/*.py, experiments): MLM_KNOBS="rank_grid=64,sec_tab=1024" -> mlm_debug_set before the first create
        for kv in os.environ["MLM_KNOBS"].split(","):
            k, _, v = kv.partition("=")
            if k.strip() and L.mlm_debug_set(k.strip().encode(), int(v)) != MLM_OK:
                raise MlmError(f"MLM_KNOBS: unknown knob {k.strip()!r} or a value the kernels cannot run: {v}")
    if path is None:
        _lib = L
    return L


def _p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def debug_set(name: str, value: int):
    """Test / experiment knob read by the next mlm_create of this process (mlm_debug_set; not part of the drop-in contract)."""
    if load_library().mlm_debug_set(name.encode(), int(value)) != MLM_OK:
        raise MlmError(f"mlm_debug_set: unknown knob {name!r} or a value the kernels cannot run: {value}")


def debug_reset():
    load_library().mlm_debug_reset()


class Delta:
    """What MLMap.delta returns: `table` = (keys, digest) of the selected blocks, the next call's prev; the changed and new blocks
    `keys`, `log_odds`, `occ`, `infl` with their `kind`; the `gone` keys; `summary`.  Everything but summary is None after a dry call.
    With packed=True `stream` holds the emitted blocks as a packed stream (MLMap.pack), and without device=True the four planes stay
    None: the stream carries them."""
    __slots__ = ("table", "keys", "log_odds", "occ", "infl", "kind", "gone", "summary", "stream")

    def __init__(self, summary):
        self.table = self.keys = self.log_odds = self.occ = self.infl = self.kind = self.gone = self.stream = None
        self.summary = summary


class MLMap:
    """One map on one MI355X (one handle = one device + one HIP stream)."""

    FREE, OCCUPIED, UNKNOWN = 1, 0, -1  # mlmap.h:109-114

    def __init__(self, cfg: MapConfig, device: int = 0, max_blocks: int = 0, max_points: int = 0,
                 record_awareness: bool = False, max_batch: int = 0):
        self.cfg = cfg
        self.cells = cfg.cells_per_block
        self.device = device
        self._L = load_library()
        self._c = to_c(cfg)
        self._lim = Limits(max_blocks, max_points, max_batch, int(record_awareness))
        self._h = ctypes.c_void_p()
        rc = self._L.mlm_create(ctypes.byref(self._c), ctypes.byref(self._lim), device, ctypes.byref(self._h))
        if rc != MLM_OK:
            msg = self._L.mlm_last_error(self._h).decode() if self._h else ""
            if self._h:
                self._L.mlm_destroy(self._h)
                self._h = ctypes.c_void_p()
            raise MlmError(f"mlm_create failed: {STATUS.get(rc, rc)} {msg}")

    # ---- lifetime -------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.mlm_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int, what: str):
        if rc != MLM_OK:
            raise MlmError(f"{what}: {STATUS.get(rc, rc)}: {self._L.mlm_last_error(self._h).decode()}")

    def set_stream(self, stream_ptr: int):
        self._chk(self._L.mlm_set_stream(self._h, ctypes.c_void_p(stream_ptr)), "mlm_set_stream")

    def sync(self):
        self._chk(self._L.mlm_sync(self._h), "mlm_sync")

    def host_register(self, arr: np.ndarray):
        """Pin a host array the host-buffer entry points will be fed from (mlm_host_register)."""
        self._chk(self._L.mlm_host_register(self._h, _p(arr), arr.nbytes), "mlm_host_register")

    def debug_clocks(self, reset: bool = True) -> np.ndarray:
        """Host clocks of the single-frame callback path, microseconds summed over the calls (mlm_debug_clocks)."""
        out = np.zeros(8)
        self._chk(self._L.mlm_debug_clocks(self._h, _p(out), int(reset)), "mlm_debug_clocks")
        return out

    def debug_probe_seeds(self) -> np.ndarray:
        """Largest relative errors of the reciprocal / reciprocal-square-root seeds and their refined forms (mlm_debug_probe_seeds)."""
        out = np.zeros(4)
        self._chk(self._L.mlm_debug_probe_seeds(self._h, _p(out)), "mlm_debug_probe_seeds")
        return out

    def host_unregister(self, arr: np.ndarray):
        self._chk(self._L.mlm_host_unregister(self._h, _p(arr)), "mlm_host_unregister")

    def set_async(self, on: bool = True):
        """Integrate calls return after submission (two batches in flight); sync()/queries wait for everything."""
        self._chk(self._L.mlm_set_async(self._h, int(on)), "mlm_set_async")

    def set_host_mirror_limit(self, max_bytes: int):
        """Most pinned host memory the mirror of the map (small query batches) may take; 0 = queries always run as kernels."""
        self._chk(self._L.mlm_set_host_mirror_limit(self._h, int(max_bytes)), "mlm_set_host_mirror_limit")

    # ---- update_map (mlmap.cpp:382-386) ---------------------------------------------------------
    def update_map(self, depth_u16: np.ndarray, q_wb, t_wb, pixel_idx=None):
        """project_depth + update_map on a host uint16 depth image (mm).  ``pixel_idx`` (v*W+u) reproduces a
        sampler; None = dense."""
        img = np.ascontiguousarray(depth_u16, dtype=np.uint16)
        hgt, wid = img.shape
        if pixel_idx is None:
            pp, n = None, 0
        else:
            pix = np.ascontiguousarray(pixel_idx, dtype=np.int32)
            pp, n = _p(pix), pix.size
        self._chk(self._L.mlm_integrate_depth_u16(self._h, _p(img), wid, hgt, wid, pp, n, _p(_f64(q_wb)),
                                                  _p(_f64(t_wb))), "mlm_integrate_depth_u16")

    def update_map_dev(self, img_dev_ptr: int, width: int, height: int, q_wb, t_wb, row_stride: int = 0):
        """Same with the image already in HBM (device pointer)."""
        self._chk(self._L.mlm_integrate_depth_u16_dev(self._h, ctypes.c_void_p(img_dev_ptr), width, height,
                                                      row_stride or width, None, 0, _p(_f64(q_wb)), _p(_f64(t_wb))),
                  "mlm_integrate_depth_u16_dev")

    def update_map_batch_dev(self, img_dev_ptr: int, n_frames: int, width: int, height: int, q_wb, t_wb,
                             frame_stride: int = 0, row_stride: int = 0):
        q = _f64(q_wb).reshape(n_frames, 4)
        t = _f64(t_wb).reshape(n_frames, 3)
        self._chk(self._L.mlm_integrate_depth_batch_dev(self._h, ctypes.c_void_p(img_dev_ptr), n_frames,
                                                        frame_stride or (row_stride or width) * height, width, height,
                                                        row_stride or width, _p(q), _p(t)),
                  "mlm_integrate_depth_batch_dev")

    def update_map_batch(self, frames_u16: np.ndarray, q_wb, t_wb):
        """K host frames [K,H,W] of one stream, integrated in order (uploads overlap with compute)."""
        fr = np.ascontiguousarray(frames_u16, dtype=np.uint16)
        k, hgt, wid = fr.shape
        q = _f64(q_wb).reshape(k, 4)
        t = _f64(t_wb).reshape(k, 3)
        self._chk(self._L.mlm_integrate_depth_batch(self._h, _p(fr), k, hgt * wid, wid, hgt, wid, _p(q), _p(t)),
                  "mlm_integrate_depth_batch")

    def depth_odom_callback(self, depth, t_img, odom_p, odom_q, odom_v, t_odom, imu_w, t_imu, latency, sampled=True):
        """mlmap::depth_odom_input_callback (mlmap.cpp:463-532) without ROS; depth float32 metres (32FC1) or uint16 mm.
        Returns the latency-compensated T_wb as (q (w,x,y,z), t) in one array of 7."""
        d = np.ascontiguousarray(depth)
        is_f32 = int(d.dtype == np.float32)
        if not is_f32:
            d = np.ascontiguousarray(d, dtype=np.uint16)  # (no copy when it is uint16 already)
        out = np.empty(7)
        self._chk(self._L.mlm_integrate_callback(self._h, _p(d), is_f32, d.shape[1], d.shape[0], float(t_img),
                                                 _p(_f64(odom_p)), _p(_f64(odom_q)), _p(_f64(odom_v)), float(t_odom),
                                                 _p(_f64(imu_w)), float(t_imu), float(latency), int(sampled), _p(out)),
                  "mlm_integrate_callback")
        return out

    def update_map_points(self, xyz_s, q_wb, t_wb):
        """input_pc_pose(PC_s, T_wb) + input_pc_pose_direct on explicit sensor-frame points."""
        xyz = _f64(xyz_s).reshape(-1, 3)
        self._chk(self._L.mlm_integrate_points(self._h, _p(xyz), xyz.shape[0], _p(_f64(q_wb)), _p(_f64(t_wb))),
                  "mlm_integrate_points")

    # ---- queries (mlmap.h:142-295) --------------------------------------------------------------
    def getOccupancy(self, pos_w, inflate: Optional[float] = None) -> np.ndarray:
        pos = _f64(pos_w).reshape(-1, 3)
        out = np.empty(pos.shape[0], dtype=np.int8)
        if inflate is None:
            self._chk(self._L.mlm_query_occupancy(self._h, _p(pos), pos.shape[0], _p(out)), "mlm_query_occupancy")
        else:
            self._chk(self._L.mlm_query_occupancy_inflate(self._h, _p(pos), pos.shape[0], ctypes.c_float(inflate),
                                                          _p(out)), "mlm_query_occupancy_inflate")
        return out.astype(np.int32)

    def getInflateOccupancy(self, pos_w) -> np.ndarray:
        pos = _f64(pos_w).reshape(-1, 3)
        out = np.empty(pos.shape[0], dtype=np.int8)
        self._chk(self._L.mlm_query_inflate_occupancy(self._h, _p(pos), pos.shape[0], _p(out)),
                  "mlm_query_inflate_occupancy")
        return out.astype(np.int32)

    def getOdd(self, pos_w) -> np.ndarray:
        pos = _f64(pos_w).reshape(-1, 3)
        out = np.empty(pos.shape[0], dtype=np.float32)
        self._chk(self._L.mlm_query_odds(self._h, _p(pos), pos.shape[0], _p(out)), "mlm_query_odds")
        return out

    def getOddAt(self, glb_id, subbox_id) -> np.ndarray:
        """float getOdd(const Vec3I &glb_id, size_t subbox_id), mlmap.h:227-235."""
        g = np.ascontiguousarray(glb_id, dtype=np.int32).reshape(-1, 3)
        c = np.ascontiguousarray(subbox_id, dtype=np.int32).reshape(-1)
        out = np.empty(g.shape[0], dtype=np.float32)
        self._chk(self._L.mlm_query_odds_at(self._h, _p(g), _p(c), g.shape[0], _p(out)), "mlm_query_odds_at")
        return out

    def getOddGrad(self, pos_w, max_iter: int = 5) -> np.ndarray:
        pos = _f64(pos_w).reshape(-1, 3)
        out = np.empty((pos.shape[0], 3), dtype=np.float64)
        self._chk(self._L.mlm_query_odd_grad(self._h, _p(pos), pos.shape[0], max_iter, _p(out)), "mlm_query_odd_grad")
        return out

    def setFree_map_in_bound(self, box_min, box_max):
        self._merge_base = None  # (the map no longer is "merged map + own observations": see merge.merge_device_maps)
        self._chk(self._L.mlm_set_free_in_bound(self._h, _p(_f64(box_min)), _p(_f64(box_max))),
                  "mlm_set_free_in_bound")

    def inflate_map(self, ct_pos):
        self._chk(self._L.mlm_inflate_map(self._h, _p(_f64(ct_pos))), "mlm_inflate_map")

    # ---- read-out -------------------------------------------------------------------------------
    def frame_stats(self) -> Dict[str, int]:
        s = FrameStats()
        self._chk(self._L.mlm_get_frame_stats(self._h, ctypes.byref(s)), "mlm_get_frame_stats")
        return s.as_dict()

    def block_count(self) -> int:
        n = ctypes.c_int32()
        self._chk(self._L.mlm_block_count(self._h, ctypes.byref(n)), "mlm_block_count")
        return n.value

    def export_blocks(self, raw: bool = False) -> Dict[str, np.ndarray]:
        """observed_group_map contents sorted by block key (same dict layout as the oracle binding); raw=True: in the pool's slot
        order, as mlm_export_blocks writes them."""
        n, C = self.block_count(), self.cells
        keys = np.empty((n, 3), dtype=np.int32)
        lo = np.empty((n, C), dtype=np.float32)
        occ = np.empty((n, C), dtype=np.uint8)
        infl = np.empty((n, C), dtype=np.uint8)
        m = ctypes.c_int32()
        self._chk(self._L.mlm_export_blocks(self._h, n, _p(keys), _p(lo), _p(occ), _p(infl), ctypes.byref(m)),
                  "mlm_export_blocks")
        col = np.zeros(n, dtype=np.uint8)
        self._chk(self._L.mlm_export_block_flags(self._h, n, _p(col), ctypes.byref(m)), "mlm_export_block_flags")
        o = np.arange(n) if raw else np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
        return {"keys": keys[o], "collapsed": col[o], "log_odds": lo[o], "occ": occ[o], "infl": infl[o]}

    def export_frontier(self) -> np.ndarray:
        """[n,4] int32 (gx,gy,gz,cell id) of the frontier cells, sorted."""
        n = ctypes.c_int32()
        self._chk(self._L.mlm_export_frontier(self._h, 0, None, ctypes.byref(n)), "mlm_export_frontier")
        out = np.empty((n.value, 4), dtype=np.int32)
        if n.value:
            self._chk(self._L.mlm_export_frontier(self._h, n.value, _p(out), ctypes.byref(n)), "mlm_export_frontier")
        return out[np.lexsort((out[:, 3], out[:, 2], out[:, 1], out[:, 0]))]

    def frontier_points(self) -> np.ndarray:
        """float32 [n,3] centres of the frontier cells: the PointCloud2 payload of /frontier (rviz_vis.cpp:267-293)."""
        n = ctypes.c_int32()
        self._chk(self._L.mlm_export_frontier_points(self._h, 0, None, ctypes.byref(n)), "mlm_export_frontier_points")
        out = np.empty((n.value, 3), dtype=np.float32)
        if n.value:
            self._chk(self._L.mlm_export_frontier_points(self._h, n.value, _p(out), ctypes.byref(n)),
                      "mlm_export_frontier_points")
        return out

    def import_blocks(self, keys, log_odds=None, occ=None, infl=None, collapsed=None):
        """Load blocks (layout of export_blocks) into the map; host numpy arrays or device pointers (ints)."""
        def ptr(a, dt):
            if a is None:
                return None, None
            if isinstance(a, int):
                return ctypes.c_void_p(a), None
            arr = np.ascontiguousarray(a, dtype=dt)
            return _p(arr), arr
        if isinstance(keys, tuple):  # (device pointer, n)
            kp, n, keep = ctypes.c_void_p(keys[0]), int(keys[1]), None
        else:
            keep = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1, 3)
            kp, n = _p(keep), keep.shape[0]
        self._merge_base = None  # (a foreign import invalidates the baseline of periodic merges; merge_device_maps sets its own afterwards)
        holds = [ptr(log_odds, np.float32), ptr(occ, np.uint8), ptr(infl, np.uint8), ptr(collapsed, np.uint8)]
        self._chk(self._L.mlm_import_blocks(self._h, n, kp, holds[0][0], holds[1][0], holds[2][0], holds[3][0]),
                  "mlm_import_blocks")

    def crop_blocks(self, key_lo, key_dims, inside: bool = False, dry: bool = False, shrink: bool = False, out=None) -> Dict[str, np.ndarray]:
        """Drop the blocks whose key lies outside (inside=True: inside) the box key_lo <= key < key_lo + key_dims of block keys, in
        place on the device (mlm_crop_blocks).  out=None: the blocks are just dropped; out=True: they are paged out into host arrays
        sized by a dry call and returned as "keys", "log_odds", "occ", "infl", "collapsed" (what import_blocks takes to bring them
        back), in ascending order of their old slot; out={"cap": blocks, "keys": ptr, "log_odds": ptr, ...}: into device memory (ints,
        any of them may be missing).  dry=True only counts.  shrink=True gives pool memory back afterwards.  Always returns
        "summary": int64 [blocks before, kept, dropped, written, capacity before, after, device_bytes before, after]."""
        lo_a = np.ascontiguousarray(key_lo, dtype=np.int32).reshape(3)
        dims_a = np.ascontiguousarray(key_dims, dtype=np.int32).reshape(3)
        flags = (MLM_CROP_INSIDE if inside else MLM_CROP_OUTSIDE) | (MLM_CROP_DRY if dry else 0) | (MLM_CROP_SHRINK if shrink else 0)
        summary = np.zeros(MLM_CROP_ROW, dtype=np.int64)
        names = ("keys", "log_odds", "occ", "infl", "collapsed")
        res, cap, ptr = {"summary": summary}, 0, [None] * 5
        if out is True and not dry:
            self._chk(self._L.mlm_crop_blocks(self._h, _p(lo_a), _p(dims_a), flags | MLM_CROP_DRY, 0, None, None, None, None, None, _p(summary)),
                      "mlm_crop_blocks")
            cap, C = int(summary[2]), self.cells
            res.update(keys=np.empty((cap, 3), dtype=np.int32), log_odds=np.empty((cap, C), dtype=np.float32),
                       occ=np.empty((cap, C), dtype=np.uint8), infl=np.empty((cap, C), dtype=np.uint8), collapsed=np.empty(cap, dtype=np.uint8))
            ptr = [_p(res[k]) for k in names]
        elif out is not None:
            cap = int(out["cap"])
            ptr = [None if out.get(k) is None else ctypes.c_void_p(int(out[k])) for k in names]
        if not dry:
            self._merge_base = None  # (as import_blocks: the baseline of periodic merges no longer describes this map)
        self._chk(self._L.mlm_crop_blocks(self._h, _p(lo_a), _p(dims_a), flags, cap, *ptr, _p(summary)), "mlm_crop_blocks")
        return res

    def warp_blocks(self, T_sd, key_lo=None, key_dims=None, seen: bool = False, dry: bool = False, replace: bool = False,
                    out=None) -> Dict[str, np.ndarray]:
        """The map resampled under the rigid transform T_sd (12 float64: R row major, then o; it maps a point of the new frame to the
        map's frame), nearest voxel, exact (mlm_warp_blocks): the blocks of the new frame's lattice that hold a live voxel, inside the
        box key_lo <= key < key_lo + key_dims of block keys if one is given, in ascending key order.  out=None: nothing is written;
        out=True: host arrays sized by a dry call, returned as "keys", "log_odds", "occ", "infl" (what import_blocks takes);
        out={"cap": blocks, "keys": ptr, "log_odds": ptr, ...}: device memory (ints, any of them may be missing).  seen=True: only
        voxels the map has observed or inflated are live.  dry=True only counts.  replace=True: afterwards this handle holds the warped
        map (not in frontier mode).  Always returns "summary": int64 [source blocks, candidates examined, emitted, written, live voxels,
        live with occ 'o', with occ 'f', with infl 'o']."""
        T = np.ascontiguousarray(_f64(T_sd).reshape(12))
        if (key_lo is None) != (key_dims is None):
            raise MlmError("warp_blocks: key_lo and key_dims go together")
        lo_a = None if key_lo is None else np.ascontiguousarray(key_lo, dtype=np.int32).reshape(3)
        dims_a = None if key_dims is None else np.ascontiguousarray(key_dims, dtype=np.int32).reshape(3)
        box = (None, None) if lo_a is None else (_p(lo_a), _p(dims_a))
        flags = (MLM_WARP_SEEN if seen else 0) | (MLM_WARP_DRY if dry else 0) | (MLM_WARP_REPLACE if replace else 0)
        summary = np.zeros(MLM_WARP_ROW, dtype=np.int64)
        names = ("keys", "log_odds", "occ", "infl")
        res, cap, ptr = {"summary": summary}, 0, [None] * 4
        if out is True and not dry:
            self._chk(self._L.mlm_warp_blocks(self._h, _p(T), *box, (flags | MLM_WARP_DRY) & ~MLM_WARP_REPLACE, 0, None, None, None, None, _p(summary)),
                      "mlm_warp_blocks")
            cap, C = int(summary[2]), self.cells
            res.update(keys=np.empty((cap, 3), dtype=np.int32), log_odds=np.empty((cap, C), dtype=np.float32),
                       occ=np.empty((cap, C), dtype=np.uint8), infl=np.empty((cap, C), dtype=np.uint8))
            ptr = [_p(res[k]) for k in names]
        elif out is not None and out is not True:
            cap = int(out["cap"])
            ptr = [None if out.get(k) is None else ctypes.c_void_p(int(out[k])) for k in names]
        if replace and not dry:
            self._merge_base = None  # (as import_blocks: the baseline of periodic merges no longer describes this map)
        self._chk(self._L.mlm_warp_blocks(self._h, _p(T), *box, flags, cap, *ptr, _p(summary)), "mlm_warp_blocks")
        return res

    def fuse_blocks(self, keys, log_odds, occ, infl=None, mode="add", dry: bool = False, per_row: bool = False) -> Dict[str, np.ndarray]:
        """Fuse a block dump (layout of export_blocks / crop_blocks / warp_blocks; host numpy arrays or device pointers (ints), keys
        then as (device pointer, n), as import_blocks takes them) into the map in place (mlm_fuse_blocks).  mode "add": log-odds added
        and clamped, class from occupied_sh (merge.py's rule); "max": the larger log-odds; "take": the dump's; "fill": the dump's where
        the map has seen nothing.  Only voxels the dump has seen (occ 'f' / 'o') count; infl 'o' is or-ed in; blocks are created as
        needed.  dry=True changes nothing and only counts: the map diff.  Returns "summary": int64 [rows, present, created, touching
        nothing, contributing voxels, new to the map, agreeing, conflicting, turned occupied, occupied turned free, infl turned on,
        log-odds changed] and "per_row": int32 [n, 4] (contributing, conflicts, class changes, 0 present / 1 created / 2 left absent)
        or None."""
        def ptr(a, dt):
            if a is None:
                return None, None
            if isinstance(a, int):
                return ctypes.c_void_p(a), None
            arr = np.ascontiguousarray(a, dtype=dt)
            return _p(arr), arr
        if isinstance(keys, tuple):  # (device pointer, n)
            kp, n, keep = ctypes.c_void_p(keys[0]), int(keys[1]), None
        else:
            keep = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1, 3)
            kp, n = _p(keep), keep.shape[0]
        if mode not in FUSE_MODES:
            raise MlmError(f"fuse_blocks: mode must be one of {sorted(FUSE_MODES)}")
        holds = [ptr(log_odds, np.float32), ptr(occ, np.uint8), ptr(infl, np.uint8)]
        summary = np.zeros(MLM_FUSE_ROW, dtype=np.int64)
        rows = np.zeros((n, MLM_FUSE_COLS), dtype=np.int32) if per_row else None
        if not dry:
            self._merge_base = None  # (as import_blocks: the baseline of periodic merges no longer describes this map)
        self._chk(self._L.mlm_fuse_blocks(self._h, n, kp, holds[0][0], holds[1][0], holds[2][0], FUSE_MODES[mode], MLM_FUSE_DRY if dry else 0,
                                          None if rows is None else _p(rows), _p(summary)), "mlm_fuse_blocks")
        return {"summary": summary, "per_row": rows}

    def fuse_from(self, other: "MLMap", T_sd=None, mode="add", dry: bool = False) -> Dict[str, np.ndarray]:
        """Fuse another handle's map into this one without the dump leaving the device: other.warp_blocks(T_sd, seen=True) into torch
        tensors on this handle's device, sized by a dry call, then fuse_blocks on their pointers.  T_sd (12 float64: R row major, then
        o; None: the identity) maps a point of THIS map's frame to other's, warp_blocks' convention.  Returns fuse_blocks' dict."""
        import torch

        T = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=np.float64) if T_sd is None else np.ascontiguousarray(_f64(T_sd).reshape(12))
        E, C = int(other.warp_blocks(T, seen=True, dry=True)["summary"][2]), self.cells
        if other.cells != C:
            raise MlmError("fuse_from: the two maps differ in subbox_n")
        dev = torch.device("cuda", self.device)
        t = {"keys": torch.empty((max(E, 1), 3), dtype=torch.int32, device=dev), "log_odds": torch.empty((max(E, 1), C), dtype=torch.float32, device=dev),
             "occ": torch.empty((max(E, 1), C), dtype=torch.uint8, device=dev), "infl": torch.empty((max(E, 1), C), dtype=torch.uint8, device=dev)}
        torch.cuda.synchronize(dev)
        if E:
            other.warp_blocks(T, seen=True, out={"cap": E, **{k: v.data_ptr() for k, v in t.items()}})
        return self.fuse_blocks((t["keys"].data_ptr(), E), t["log_odds"].data_ptr(), t["occ"].data_ptr(), t["infl"].data_ptr(), mode=mode, dry=dry)

    def reanchor(self, T_ds) -> Dict[str, np.ndarray]:
        """Apply a frame correction to the map in place: T_ds (12 float64: R row major, then t) maps a point of the map's current frame
        to the corrected one, as a caller thinks of a correction (new-from-old).  It is inverted here (invert_T) and handed to
        warp_blocks(replace=True), whose "summary" is returned."""
        return self.warp_blocks(invert_T(T_ds), replace=True)

    def retain_around(self, t_w, radius_m: float, shrink: bool = False, out=None) -> Dict[str, np.ndarray]:
        """Keep a rolling window: drop every block farther than radius_m from t_w on some axis — the kept key box is
        floor((t - r) / d_glb) - 1 .. floor((t + r) / d_glb) + 1 per axis (one block of margin).  See crop_blocks."""
        lo, dims = self.retain_box(t_w, radius_m)
        return self.crop_blocks(lo, dims, inside=False, shrink=shrink, out=out)

    def retain_box(self, t_w, radius_m: float):
        """retain_around's and age_outside's key box as (key_lo, key_dims): floor((t - r) / d_glb) - 1 .. floor((t + r) / d_glb) + 1."""
        t = _f64(t_w).reshape(3)
        d_glb = self.cfg.subbox_d_xyz * self.cfg.subbox_n  # (map_local.cpp:60, as mlm_create computes it)
        lo = np.floor((t - radius_m) / d_glb).astype(np.int64) - 1
        hi = np.floor((t + radius_m) / d_glb).astype(np.int64) + 1
        return lo, hi - lo + 1

    def age_blocks(self, key_lo=None, key_dims=None, mode="scale", amount: float = 1.0, forget: Optional[float] = None, outside: bool = False,
                   drop: bool = False, clear_infl: bool = False, dry: bool = False, per_block=False) -> Dict[str, np.ndarray]:
        """Age the map in place on the device (mlm_age_blocks): in the blocks whose key lies inside the box key_lo <= key < key_lo +
        key_dims (outside=True: outside it; no box: in every block) every voxel that holds a class or evidence gets its log-odds scaled
        by amount (mode "scale", amount in [0, 1]) or moved towards zero by amount (mode "step"), clamped, and its class set from
        occupied_sh; with forget=x a voxel whose |log-odds| <= x afterwards goes back to unknown; clear_infl=True resets the inflation of
        the selected blocks; drop=True drops the selected blocks that are empty afterwards, as crop_blocks drops blocks.  dry=True
        changes nothing and only counts.  per_block=True: also "per_block", int32 [blocks before, 4] by old slot (aged, forgotten, class
        changes, 0 not selected / 1 kept / 2 empty: dropped); per_block=<int>: a device pointer to that many rows, written in place.
        Returns "summary": int64 [blocks before, selected, dropped, afterwards, aged voxels, log-odds changed, forgotten, forgotten
        'o', forgotten 'f', 'o' -> 'f', 'f' -> 'o', infl cleared]."""
        if (key_lo is None) != (key_dims is None):
            raise MlmError("age_blocks: key_lo and key_dims go together")
        if mode not in AGE_MODES:
            raise MlmError(f"age_blocks: mode must be one of {sorted(AGE_MODES)}")
        lo_a = None if key_lo is None else np.ascontiguousarray(key_lo, dtype=np.int32).reshape(3)
        dims_a = None if key_dims is None else np.ascontiguousarray(key_dims, dtype=np.int32).reshape(3)
        box = (None, None) if lo_a is None else (_p(lo_a), _p(dims_a))
        flags = ((MLM_AGE_OUTSIDE if outside else 0) | (MLM_AGE_DRY if dry else 0) | (MLM_AGE_FORGET if forget is not None else 0) |
                 (MLM_AGE_DROP if drop else 0) | (MLM_AGE_CLEAR_INFL if clear_infl else 0))
        summary = np.zeros(MLM_AGE_ROW, dtype=np.int64)
        rows, pb = None, None
        if per_block is True:
            rows = np.zeros((self.block_count(), MLM_AGE_COLS), dtype=np.int32)
            pb = _p(rows)
        elif per_block is not False and per_block is not None:
            pb = ctypes.c_void_p(int(per_block))
        if not dry:
            self._merge_base = None  # (as import_blocks: the baseline of periodic merges no longer describes this map)
        self._chk(self._L.mlm_age_blocks(self._h, *box, AGE_MODES[mode], float(amount), 0.0 if forget is None else float(forget), flags, pb, _p(summary)),
                  "mlm_age_blocks")
        return {"summary": summary, "per_block": rows}

    def age_outside(self, t_w, radius_m: float, **kw) -> Dict[str, np.ndarray]:
        """Age everything but where the sensor is looking: age_blocks(outside=True) with retain_around's key box for the same t_w and
        radius_m.  See age_blocks for the other arguments."""
        lo, dims = self.retain_box(t_w, radius_m)
        return self.age_blocks(lo, dims, outside=True, **kw)

    def delta(self, prev=None, box=None, no_infl: bool = False, dry: bool = False, device: bool = False, packed: bool = False) -> "Delta":
        """Which blocks differ from the last time the caller looked (mlm_delta_blocks).  prev: the `table` (keys int32 [n, 3], digest
        uint64 [n, 2]) an earlier call returned, or that call's Delta, as numpy arrays or torch tensors on this handle's device; None:
        everything is new.  box: (key_lo, key_dims) of block keys, None: every block.  no_infl=True: infl reads as 'u' and is never a
        difference.  The outputs are sized by a dry call; dry=True stops there (only `summary` is filled).  Returns a Delta: `table` (the
        next call's prev), the changed and new blocks `keys`, `log_odds`, `occ`, `infl` in import_blocks' layout with `kind` (1 changed, 2
        new), the `gone` keys and `summary`: int64 [blocks, selected, n_prev, prev rows inside the box, unchanged, changed, new, gone,
        blocks written, table rows written, gone keys written, empty selected blocks] — numpy arrays, or with device=True torch tensors
        on this handle's device (digest as int64: the same bits).  packed=True: the emitted blocks go into device tensors and from there
        into `stream`, a packed stream (pack; a numpy uint8 array, or with device=True a device tensor); without device=True `keys`,
        `log_odds`, `occ`, `infl` stay None (apply_delta takes the stream)."""
        if isinstance(prev, Delta):
            prev = prev.table
        hold = []

        def ptr(a, dt):  # numpy array or torch tensor -> pointer
            if hasattr(a, "data_ptr"):
                t = a.contiguous()
                hold.append(t)
                return ctypes.c_void_p(t.data_ptr()) if t.numel() else None
            arr = np.ascontiguousarray(a, dtype=dt)
            hold.append(arr)
            return _p(arr) if arr.size else None
        n_prev, pk, pd = 0, None, None
        if prev is not None:
            n_prev = int(prev[0].shape[0]) if hasattr(prev[0], "shape") else len(prev[0])
            if n_prev:
                pk, pd = ptr(prev[0], np.int32), ptr(prev[1], np.uint64)
        lo_a = dims_a = None
        if box is not None:
            lo_a = np.ascontiguousarray(box[0], dtype=np.int32).reshape(3)
            dims_a = np.ascontiguousarray(box[1], dtype=np.int32).reshape(3)
        bx = (None, None) if lo_a is None else (_p(lo_a), _p(dims_a))
        flags = MLM_DELTA_NO_INFL if no_infl else 0
        summary = np.zeros(MLM_DELTA_ROW, dtype=np.int64)
        self._chk(self._L.mlm_delta_blocks(self._h, *bx, n_prev, pk, pd, flags | MLM_DELTA_DRY, 0, None, None, 0, None, None, None, None, None, 0, None, _p(summary)),
                  "mlm_delta_blocks")
        d = Delta(summary=summary)
        if dry:
            return d
        S, E, G, C = int(summary[1]), int(summary[5] + summary[6]), int(summary[7]), self.cells
        shapes = (("tk", (S, 3), np.int32), ("td", (S, 2), np.uint64), ("keys", (E, 3), np.int32), ("log_odds", (E, C), np.float32), ("occ", (E, C), np.uint8),
                  ("infl", (E, C), np.uint8), ("kind", (E,), np.uint8), ("gone", (G, 3), np.int32))
        on_dev = {k for k, _, _ in shapes} if device else {"keys", "log_odds", "occ", "infl"} if packed else set()
        out = {k: np.empty(shape, dtype=dt) for k, shape, dt in shapes if k not in on_dev}
        p = {k: _p(v) if v.size else None for k, v in out.items()}
        if on_dev:
            import torch

            dev = torch.device("cuda", self.device)
            tt = {np.int32: torch.int32, np.uint64: torch.int64, np.float32: torch.float32, np.uint8: torch.uint8}
            out.update({k: torch.empty(shape, dtype=tt[dt], device=dev) for k, shape, dt in shapes if k in on_dev})
            torch.cuda.synchronize(dev)
            p.update({k: ctypes.c_void_p(out[k].data_ptr()) if out[k].numel() else None for k in on_dev})
        self._chk(self._L.mlm_delta_blocks(self._h, *bx, n_prev, pk, pd, flags, S, p["tk"], p["td"], E, p["keys"], p["log_odds"], p["occ"], p["infl"], p["kind"],
                                           G, p["gone"], _p(summary)), "mlm_delta_blocks")
        d.table = (out["tk"], out["td"])
        d.keys, d.log_odds, d.occ, d.infl, d.kind, d.gone = (out[k] for k in ("keys", "log_odds", "occ", "infl", "kind", "gone"))
        if packed:
            d.stream = self.pack(rows=(d.keys, d.log_odds, d.occ, d.infl), no_infl=no_infl, device=device)
            if not device:
                d.keys = d.log_odds = d.occ = d.infl = None
        return d

    def apply_delta(self, d: "Delta"):
        """Make this handle — a replica of the one d came from — follow: import_blocks of the emitted blocks (whole blocks are
        overwritten or created), then one crop_blocks(inside=True) with a one-key box per gone key (a crop by key list is not built).
        d's arrays may be numpy arrays or torch tensors on this handle's device; a Delta that carries only `stream` (delta(packed=True))
        is unpacked into device tensors first."""
        if d.keys is None and d.stream is not None:
            rows = self.unpack(d.stream, device=True)
            n = int(rows["keys"].shape[0])
            if n:
                self.import_blocks((rows["keys"].data_ptr(), n), rows["log_odds"].data_ptr(), rows["occ"].data_ptr(), rows["infl"].data_ptr())
            gone = d.gone.cpu().numpy() if hasattr(d.gone, "cpu") else np.asarray(d.gone)
            for k in gone.reshape(-1, 3):
                self.crop_blocks(k, [1, 1, 1], inside=True)
            return
        n = int(d.keys.shape[0])
        if n:
            if hasattr(d.keys, "data_ptr"):
                self.import_blocks((d.keys.data_ptr(), n), d.log_odds.data_ptr(), d.occ.data_ptr(), d.infl.data_ptr())
            else:
                self.import_blocks(d.keys, d.log_odds, d.occ, d.infl)
        gone = d.gone.cpu().numpy() if hasattr(d.gone, "cpu") else np.asarray(d.gone)
        for k in gone.reshape(-1, 3):
            self.crop_blocks(k, [1, 1, 1], inside=True)

    def pack(self, box=None, rows=None, no_infl: bool = False, device: bool = False):
        """The lossless packed stream (mlm_pack_blocks; the format: include/mlmap_hip.h) of the live map's blocks — of the key box
        box = (key_lo, key_dims), None: of every block, ascending by key — or of rows = (keys, log_odds, occ, infl) of a dump in
        import_blocks' layout, in their order (numpy arrays or torch tensors on this handle's device; infl may be None).  no_infl=True:
        infl reads 'u'.  Sized by a dry call; returns a numpy uint8 array, or with device=True a torch uint8 tensor on this handle's
        device.  `pack_summary` holds the last call's summary: int64 [blocks, stream bytes, raw bytes, blank blocks, literals, cells on
        log_odds_min, cells on log_odds_max, bytes written]."""
        hold = []

        def ptr(a, dt):
            if a is None:
                return None
            if hasattr(a, "data_ptr"):
                t = a.contiguous()
                hold.append(t)
                return ctypes.c_void_p(t.data_ptr()) if t.numel() else None
            arr = np.ascontiguousarray(a, dtype=dt)
            hold.append(arr)
            return _p(arr) if arr.size else None
        bx, n, src = (None, None), 0, (None, None, None, None)
        if rows is not None:
            if box is not None:
                raise MlmError("pack: a box selects blocks of the live map, it does not go with rows")
            n = int(rows[0].shape[0])
            one = np.zeros(3, dtype=np.int32)  # (zero rows: still the rows source, so a pointer that is not NULL)
            hold.append(one)
            src = tuple(ptr(a, dt) for a, dt in zip(rows, (np.int32, np.float32, np.uint8, np.uint8)))
            if n == 0:
                src = (_p(one), None, None, None)
        elif box is not None:
            lo_a = np.ascontiguousarray(box[0], dtype=np.int32).reshape(3)
            dims_a = np.ascontiguousarray(box[1], dtype=np.int32).reshape(3)
            hold += [lo_a, dims_a]
            bx = (_p(lo_a), _p(dims_a))
        flags = MLM_PACK_NO_INFL if no_infl else 0
        summary = np.zeros(MLM_PACK_ROW, dtype=np.int64)
        self._chk(self._L.mlm_pack_blocks(self._h, *bx, n, *src, flags | MLM_PACK_DRY, 0, None, _p(summary)), "mlm_pack_blocks")
        size = int(summary[1])
        if device:
            import torch

            dev = torch.device("cuda", self.device)
            out = torch.empty(size, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            op = ctypes.c_void_p(out.data_ptr())
        else:
            out = np.empty(size, dtype=np.uint8)
            op = _p(out)
        self._chk(self._L.mlm_pack_blocks(self._h, *bx, n, *src, flags, size, op, _p(summary)), "mlm_pack_blocks")
        self.pack_summary = summary
        return out

    def unpack(self, stream, device: bool = False) -> Dict[str, np.ndarray]:
        """A packed stream (bytes, a numpy uint8 array or a torch uint8 tensor on this handle's device) back into rows (mlm_unpack_blocks):
        "keys" int32 [n, 3], "log_odds" float32 [n, C], "occ", "infl" uint8 [n, C] in import_blocks' layout — numpy arrays, or with
        device=True torch tensors on this handle's device — and "summary".  The stream is validated whole before anything is written;
        a stream that is not one raises MlmError with the number of the failed check."""
        if hasattr(stream, "data_ptr"):
            keep = stream.contiguous()
            sp, size = ctypes.c_void_p(keep.data_ptr()), int(keep.numel())
        else:
            keep = np.frombuffer(stream, dtype=np.uint8) if isinstance(stream, (bytes, bytearray, memoryview)) else np.ascontiguousarray(stream, dtype=np.uint8)
            sp, size = _p(keep), int(keep.size)
        if size == 0:
            keep = np.zeros(1, dtype=np.uint8)
            sp = _p(keep)
        summary = np.zeros(MLM_PACK_ROW, dtype=np.int64)
        self._chk(self._L.mlm_unpack_blocks(self._h, sp, size, 0, 0, None, None, None, None, _p(summary)), "mlm_unpack_blocks")
        n, C = int(summary[0]), self.cells
        shapes = (("keys", (n, 3), np.int32), ("log_odds", (n, C), np.float32), ("occ", (n, C), np.uint8), ("infl", (n, C), np.uint8))
        if device:
            import torch

            dev = torch.device("cuda", self.device)
            tt = {np.int32: torch.int32, np.float32: torch.float32, np.uint8: torch.uint8}
            out = {k: torch.empty(shape, dtype=tt[dt], device=dev) for k, shape, dt in shapes}
            torch.cuda.synchronize(dev)
            p = [ctypes.c_void_p(out[k].data_ptr()) if n else None for k, _, _ in shapes]
        else:
            out = {k: np.empty(shape, dtype=dt) for k, shape, dt in shapes}
            p = [_p(out[k]) if n else None for k, _, _ in shapes]
        if n:
            self._chk(self._L.mlm_unpack_blocks(self._h, sp, size, 0, n, *p, _p(summary)), "mlm_unpack_blocks")
        out["summary"] = summary
        return out

    def save(self, path, box=None, no_infl: bool = False) -> int:
        """The map (its blocks of the key box, if one is given) as a packed stream in a file; returns the bytes written.  See pack."""
        stream = self.pack(box=box, no_infl=no_infl)
        with open(path, "wb") as f:
            f.write(stream.tobytes())
        return int(stream.size)

    def load(self, path, fuse: Optional[str] = None) -> Dict[str, np.ndarray]:
        """A file save wrote, brought into this map: unpacked into device tensors (the dump never exists on the host), then
        import_blocks — whole blocks are overwritten or created — or, with fuse="add" / "max" / "take" / "fill", fuse_blocks with that
        mode.  Returns unpack's "summary" (and fuse_blocks' dict under "fuse")."""
        rows = self.unpack(np.fromfile(path, dtype=np.uint8), device=True)
        n = int(rows["keys"].shape[0])
        res = {"summary": rows["summary"]}
        if n and fuse is None:
            self.import_blocks((rows["keys"].data_ptr(), n), rows["log_odds"].data_ptr(), rows["occ"].data_ptr(), rows["infl"].data_ptr())
        elif n:
            res["fuse"] = self.fuse_blocks((rows["keys"].data_ptr(), n), rows["log_odds"].data_ptr(), rows["occ"].data_ptr(), rows["infl"].data_ptr(), mode=fuse)
        return res

    def export_window(self, lo, dims, odds=True, occ=False, infl=False, grad=False, max_iter: int = 5) -> Dict[str, np.ndarray]:
        """Dense read-out of the voxel box lo <= v < lo + dims (voxel indices v = block key * subbox_n + cell coordinate, per axis
        (x, y, z)): {"odds": float32, "occ": int8, "infl": int8 shaped (dz, dy, dx), "grad": float64 (dz, dy, dx, 3)} for the
        channels asked for — getOdd / getOccupancy / getInflateOccupancy / getOddGrad(max_iter) at every voxel (mlm_export_window)."""
        lo_a, dims_a = self._window_args(lo, dims)
        shape = (int(dims_a[2]), int(dims_a[1]), int(dims_a[0]))
        out = {}
        if odds:
            out["odds"] = np.empty(shape, dtype=np.float32)
        if occ:
            out["occ"] = np.empty(shape, dtype=np.int8)
        if infl:
            out["infl"] = np.empty(shape, dtype=np.int8)
        if grad:
            out["grad"] = np.empty(shape + (3,), dtype=np.float64)
        ptr = [_p(out[k]) if k in out else None for k in ("odds", "occ", "infl", "grad")]
        self._chk(self._L.mlm_export_window(self._h, _p(lo_a), _p(dims_a), int(max_iter), *ptr), "mlm_export_window")
        return out

    def export_window_dev(self, lo, dims, max_iter: int = 5, odds: Optional[int] = None, occ: Optional[int] = None,
                          infl: Optional[int] = None, grad: Optional[int] = None):
        """Same into device memory: pointers (ints) to dz*dy*dx float32 / int8 / int8 / (x3) float64 elements, None = skipped."""
        lo_a, dims_a = self._window_args(lo, dims)
        ptr = [None if v is None else ctypes.c_void_p(v) for v in (odds, occ, infl, grad)]
        self._chk(self._L.mlm_export_window(self._h, _p(lo_a), _p(dims_a), int(max_iter), *ptr), "mlm_export_window")

    def export_esdf(self, lo, dims, max_dist: int, occ=True, infl=False, unknown=False, signed=False, sqdist=True, dist=False,
                    grad=False) -> Dict[str, np.ndarray]:
        """Truncated Euclidean distance field of the voxel box lo <= v < lo + dims (voxel indices as export_window): {"sqdist":
        int32, "dist": float32 shaped (dz, dy, dx), "grad": float32 (dz, dy, dx, 3)} for the channels asked for.  Obstacles are
        the union of occ (getOccupancy == OCCUPIED), infl (getInflateOccupancy == OCCUPIED) and unknown (getOccupancy == UNKNOWN);
        squared index distances to the nearest obstacle of the whole map, clamped at max_dist^2; signed: minus the distance to
        the nearest non-obstacle on obstacles (mlm_export_esdf)."""
        lo_a, dims_a = self._window_args(lo, dims)
        shape = (int(dims_a[2]), int(dims_a[1]), int(dims_a[0]))
        out = {}
        if sqdist:
            out["sqdist"] = np.empty(shape, dtype=np.int32)
        if dist:
            out["dist"] = np.empty(shape, dtype=np.float32)
        if grad:
            out["grad"] = np.empty(shape + (3,), dtype=np.float32)
        ptr = [_p(out[k]) if k in out else None for k in ("sqdist", "dist", "grad")]
        flags = self._esdf_flags(occ, infl, unknown, signed)
        self._chk(self._L.mlm_export_esdf(self._h, _p(lo_a), _p(dims_a), int(max_dist), flags, *ptr), "mlm_export_esdf")
        return out

    def export_esdf_dev(self, lo, dims, max_dist: int, occ=True, infl=False, unknown=False, signed=False,
                        sqdist: Optional[int] = None, dist: Optional[int] = None, grad: Optional[int] = None):
        """Same into device memory: pointers (ints) to dz*dy*dx int32 / float32 / (x3) float32 elements, None = skipped."""
        lo_a, dims_a = self._window_args(lo, dims)
        ptr = [None if v is None else ctypes.c_void_p(v) for v in (sqdist, dist, grad)]
        flags = self._esdf_flags(occ, infl, unknown, signed)
        self._chk(self._L.mlm_export_esdf(self._h, _p(lo_a), _p(dims_a), int(max_dist), flags, *ptr), "mlm_export_esdf")

    def export_grid2d(self, lo, dims, occ=True, infl=False, unknown=False, min_free: int = 0, z_ref: Optional[int] = None,
                      max_dist: Optional[int] = None, dist_unobserved=False, grid=True, cols=False, sqdist=False, dist=False) -> Dict[str, np.ndarray]:
        """The slab lo <= v < lo + dims (voxel indices as export_window) projected onto the ground plane: {"grid": int8 (dy, dx),
        100 where the column lo[2] <= z < lo[2] + dims[2] holds an obstacle, else -1 where it holds fewer than min_free FREE voxels,
        else 0 — nav_msgs/OccupancyGrid's data order; "cols": int32 (dy, dx, 8): n_obs, n_unk, n_free, lowest and highest obstacle z,
        the nearest obstacle z at or below and at or above z_ref (none: lo[2] - 1 / lo[2] + dims[2]), the UNKNOWN voxels strictly
        between those two; "sqdist": int32 and "dist": float32 (dy, dx), the plane distance to the nearest cell with grid == 100
        (dist_unobserved: grid != 0) anywhere in the plane, squared in cells and clamped at max_dist^2, and in metres; "summary":
        int64 [cells with 100, 0, -1, sum of n_obs, n_unk, n_free]}.  Obstacles are the union of occ / infl / unknown as in
        export_esdf; z_ref=None is the middle layer lo[2] + dims[2] // 2; max_dist (1..64) is needed for sqdist / dist
        (mlm_export_grid2d; grid2d_band turns a height band in metres into lo[2], dims[2] and z_ref)."""
        lo_a, dims_a = self._window_args(lo, dims)
        shape = (int(dims_a[1]), int(dims_a[0]))
        out = {}
        if grid:
            out["grid"] = np.empty(shape, dtype=np.int8)
        if cols:
            out["cols"] = np.empty(shape + (MLM_GRID_COL,), dtype=np.int32)
        if sqdist:
            out["sqdist"] = np.empty(shape, dtype=np.int32)
        if dist:
            out["dist"] = np.empty(shape, dtype=np.float32)
        out["summary"] = np.zeros(6, dtype=np.int64)
        ptr = [_p(out[k]) if k in out else None for k in ("grid", "cols", "sqdist", "dist", "summary")]
        self._chk(self._L.mlm_export_grid2d(self._h, _p(lo_a), _p(dims_a), self._grid_flags(occ, infl, unknown, dist_unobserved), int(min_free),
                                            self._grid_z_ref(lo_a, dims_a, z_ref), int(max_dist or 0), *ptr), "mlm_export_grid2d")
        return out

    def export_grid2d_dev(self, lo, dims, occ=True, infl=False, unknown=False, min_free: int = 0, z_ref: Optional[int] = None,
                          max_dist: Optional[int] = None, dist_unobserved=False, grid: Optional[int] = None, cols: Optional[int] = None,
                          sqdist: Optional[int] = None, dist: Optional[int] = None) -> np.ndarray:
        """Same into device memory: pointers (ints) to dy*dx int8 / (x8) int32 / int32 / float32 elements, None = skipped; returns
        the summary."""
        lo_a, dims_a = self._window_args(lo, dims)
        summary = np.zeros(6, dtype=np.int64)
        ptr = [None if v is None else ctypes.c_void_p(v) for v in (grid, cols, sqdist, dist)]
        self._chk(self._L.mlm_export_grid2d(self._h, _p(lo_a), _p(dims_a), self._grid_flags(occ, infl, unknown, dist_unobserved), int(min_free),
                                            self._grid_z_ref(lo_a, dims_a, z_ref), int(max_dist or 0), *ptr, _p(summary)), "mlm_export_grid2d")
        return summary

    @staticmethod
    def grid2d_band(min_z: float, max_z: float, d: float, z_vehicle: Optional[float] = None) -> Tuple[int, int, int]:
        """(lo_z, dims_z, z_ref) of export_grid2d for the height band min_z .. max_z in metres at voxel size d — the reference's keys
        projected_2d_map_min_z / projected_2d_map_max_z and subbox_d_xyz.  With z_vehicle (use_relative_height) the band is min_z +
        z_vehicle .. max_z + z_vehicle.  The slab covers the layers floor(zmin / d) .. floor(zmax / d) inclusive; z_ref is
        floor(z_vehicle / d) clamped into the slab, without z_vehicle the slab's middle layer lo_z + dims_z // 2.  Plain double
        arithmetic (Python floats): one addition, one division and one floor per bound."""
        zmin, zmax = float(min_z), float(max_z)
        if z_vehicle is not None:
            zmin, zmax = zmin + float(z_vehicle), zmax + float(z_vehicle)
        if not zmin <= zmax or not d > 0:
            raise MlmError("grid2d_band: needs min_z <= max_z and d > 0")
        lo_z, hi_z = int(np.floor(zmin / float(d))), int(np.floor(zmax / float(d)))
        dims_z = hi_z - lo_z + 1
        z_ref = lo_z + dims_z // 2 if z_vehicle is None else min(max(int(np.floor(float(z_vehicle) / float(d))), lo_z), hi_z)
        return lo_z, dims_z, z_ref

    @staticmethod
    def _grid_flags(occ, infl, unknown, dist_unobserved) -> int:
        return ((MLM_GRID_OCC if occ else 0) | (MLM_GRID_INFL if infl else 0) | (MLM_GRID_UNKNOWN if unknown else 0)
                | (MLM_GRID_DIST_UNOBSERVED if dist_unobserved else 0))

    @staticmethod
    def _grid_z_ref(lo_a, dims_a, z_ref) -> int:
        return int(lo_a[2]) + int(dims_a[2]) // 2 if z_ref is None else int(z_ref)

    def export_reach(self, lo, dims, seeds, occ=True, infl=False, unknown=False, clearance: int = 0, max_steps: Optional[int] = None,
                     steps=True, parent=False) -> Dict[str, np.ndarray]:
        """Cost-to-go through the free space of the voxel box lo <= v < lo + dims (voxel indices as export_window) from `seeds`
        (k x 3 voxel indices): {"steps": int32 (dz, dy, dx), moves of the shortest 6-connected path of traversable voxels from a
        seed, -1 where there is none (or it is longer than max_steps); "parent": uint8, the neighbour code (0: -x, 1: +x, 2: -y,
        3: +y, 4: -z, 5: +z) one step nearer a seed, 6 at seeds, 255 where steps is -1; "summary": int64 [traversable, reached,
        largest steps, sweeps]}.  Obstacles are the union of occ / infl / unknown as in export_esdf (none: no obstacles); a voxel
        is traversable if no obstacle of the map lies within `clearance` voxels (Euclidean) of it; paths stay inside the box; a
        seed that is not traversable contributes nothing (mlm_export_reach)."""
        lo_a, dims_a = self._window_args(lo, dims)
        shape = (int(dims_a[2]), int(dims_a[1]), int(dims_a[0]))
        s = np.ascontiguousarray(np.asarray(seeds, dtype=np.int32).reshape(-1, 3))
        out = {"summary": np.zeros(4, dtype=np.int64)}
        if steps:
            out["steps"] = np.empty(shape, dtype=np.int32)
        if parent:
            out["parent"] = np.empty(shape, dtype=np.uint8)
        ptr = [_p(out[k]) if k in out else None for k in ("steps", "parent", "summary")]
        self._chk(self._L.mlm_export_reach(self._h, _p(lo_a), _p(dims_a), _p(s), len(s), self._ray_flags(occ, infl, unknown), int(clearance),
                                           2 ** 31 - 1 if max_steps is None else int(max_steps), *ptr), "mlm_export_reach")
        return out

    def export_reach_dev(self, lo, dims, seeds: int, n_seeds: int, occ=True, infl=False, unknown=False, clearance: int = 0,
                         max_steps: Optional[int] = None, steps: Optional[int] = None, parent: Optional[int] = None,
                         summary: bool = False) -> Optional[np.ndarray]:
        """Same on device memory: `seeds` a pointer (int) to n_seeds x 3 int32, steps / parent pointers to dz*dy*dx int32 / uint8
        elements, None = skipped; summary=True returns the four int64 counters."""
        lo_a, dims_a = self._window_args(lo, dims)
        sm = np.zeros(4, dtype=np.int64) if summary else None
        ptr = [None if v is None else ctypes.c_void_p(v) for v in (steps, parent)] + [None if sm is None else _p(sm)]
        self._chk(self._L.mlm_export_reach(self._h, _p(lo_a), _p(dims_a), ctypes.c_void_p(seeds), int(n_seeds),
                                           self._ray_flags(occ, infl, unknown), int(clearance),
                                           2 ** 31 - 1 if max_steps is None else int(max_steps), *ptr), "mlm_export_reach")
        return sm

    def export_route(self, lo, dims, seeds, occ=True, infl=False, unknown=False, clearance: int = 0, connectivity: int = 26,
                     move_cost=(10, 14, 17), penalty=(), max_cost: Optional[int] = None, cost=True, parent=False) -> Dict[str, np.ndarray]:
        """Clearance-weighted cost field through the free space of the voxel box lo <= v < lo + dims from `seeds` (k x 3 voxel
        indices), window, obstacles, clearance and seeds as export_reach: {"cost": int32 (dz, dy, dx), the cheapest path of
        permitted moves from a seed, -1 where there is none (or it costs more than max_cost); "parent": uint8, the code (0..25)
        of the offset towards the voxel before on one cheapest path, 26 at seeds, 255 where cost is -1; "summary": int64
        [traversable, reached, largest cost, sweeps]}.  connectivity 6, 18 or 26: face, edge and corner moves at move_cost[0 / 1
        / 2], a diagonal move only where all the voxels it brushes are traversable; entering a voxel in ring k around the blocked
        voxels (obstacle distance within clearance + 1 + k) adds penalty[k] (mlm_export_route)."""
        lo_a, dims_a = self._window_args(lo, dims)
        shape = (int(dims_a[2]), int(dims_a[1]), int(dims_a[0]))
        s = np.ascontiguousarray(np.asarray(seeds, dtype=np.int32).reshape(-1, 3))
        out = {"summary": np.zeros(4, dtype=np.int64)}
        if cost:
            out["cost"] = np.empty(shape, dtype=np.int32)
        if parent:
            out["parent"] = np.empty(shape, dtype=np.uint8)
        ptr = [_p(out[k]) if k in out else None for k in ("cost", "parent", "summary")]
        self._chk(self._L.mlm_export_route(self._h, _p(lo_a), _p(dims_a), _p(s), len(s), self._ray_flags(occ, infl, unknown),
                                           *self._route_args(clearance, connectivity, move_cost, penalty, max_cost), *ptr), "mlm_export_route")
        return out

    def export_route_dev(self, lo, dims, seeds: int, n_seeds: int, occ=True, infl=False, unknown=False, clearance: int = 0,
                         connectivity: int = 26, move_cost=(10, 14, 17), penalty=(), max_cost: Optional[int] = None,
                         cost: Optional[int] = None, parent: Optional[int] = None, summary: bool = False) -> Optional[np.ndarray]:
        """Same on device memory: `seeds` a pointer (int) to n_seeds x 3 int32, cost / parent pointers to dz*dy*dx int32 / uint8
        elements, None = skipped; summary=True returns the four int64 counters."""
        lo_a, dims_a = self._window_args(lo, dims)
        sm = np.zeros(4, dtype=np.int64) if summary else None
        ptr = [None if v is None else ctypes.c_void_p(v) for v in (cost, parent)] + [None if sm is None else _p(sm)]
        self._chk(self._L.mlm_export_route(self._h, _p(lo_a), _p(dims_a), ctypes.c_void_p(seeds), int(n_seeds), self._ray_flags(occ, infl, unknown),
                                           *self._route_args(clearance, connectivity, move_cost, penalty, max_cost), *ptr), "mlm_export_route")
        return sm

    @staticmethod
    def _route_args(clearance, connectivity, move_cost, penalty, max_cost):
        """clearance, connectivity, move_cost[3], penalty, n_penalty, max_cost as mlm_export_route takes them (the arrays are kept
        alive by the returned list until the call is over)"""
        mc = np.ascontiguousarray(np.asarray(move_cost, dtype=np.int32).reshape(3))
        pen = np.ascontiguousarray(np.asarray(penalty, dtype=np.int32).reshape(-1))
        return [int(clearance), int(connectivity), _p(mc), _p(pen) if len(pen) else None, len(pen), 2 ** 31 - 1 if max_cost is None else int(max_cost)]

    def export_clusters(self, lo, dims, frontier=False, occ=False, infl=False, unknown=False, connectivity: int = 26, min_size: int = 1,
                        labels=True, cap: int = 4096) -> Dict[str, np.ndarray]:
        """Connected components of a voxel set of the box lo <= v < lo + dims (voxel indices as export_window): the frontier (FREE
        voxels with an UNKNOWN face neighbour anywhere in the map; works without frontier mode) or the union of occ / infl /
        unknown as in export_esdf.  connectivity 6, 18 or 26; components of at least min_size voxels are numbered 0 .. K-1 by
        their smallest voxel.  {"labels": int32 (dz, dy, dx), the component's number, -2 in a dropped component, -1 off the set;
        "table": int64 (min(K, cap), 16): voxels, root x y z, smallest x y z, largest x y z, sums of x - lo[0], y - lo[1],
        z - lo[2], box-face bits, 0, 0; "summary": int64 [voxels of the set, components, K, voxels in kept components, largest
        component, local passes]} (mlm_export_clusters)."""
        lo_a, dims_a = self._window_args(lo, dims)
        shape = (int(dims_a[2]), int(dims_a[1]), int(dims_a[0]))
        out = {"summary": np.zeros(6, dtype=np.int64)}
        if labels:
            out["labels"] = np.empty(shape, dtype=np.int32)
        if cap > 0:
            out["table"] = np.zeros((int(cap), MLM_CLUSTER_ROW), dtype=np.int64)
        ptr = [_p(out[k]) if k in out else None for k in ("labels", "table")]
        self._chk(self._L.mlm_export_clusters(self._h, _p(lo_a), _p(dims_a), self._cluster_flags(frontier, occ, infl, unknown), int(connectivity),
                                              int(min_size), *ptr, int(cap), _p(out["summary"])), "mlm_export_clusters")
        if cap > 0:
            out["table"] = out["table"][:min(int(out["summary"][2]), int(cap))]
        return out

    def export_clusters_dev(self, lo, dims, frontier=False, occ=False, infl=False, unknown=False, connectivity: int = 26, min_size: int = 1,
                            labels: Optional[int] = None, table: Optional[int] = None, cap: int = 0,
                            summary: bool = False) -> Optional[np.ndarray]:
        """Same on device memory: labels a pointer (int) to dz*dy*dx int32, table a pointer to cap x 16 int64, None = skipped;
        summary=True returns the six int64 counters."""
        lo_a, dims_a = self._window_args(lo, dims)
        sm = np.zeros(6, dtype=np.int64) if summary else None
        ptr = [None if v is None else ctypes.c_void_p(v) for v in (labels, table)]
        self._chk(self._L.mlm_export_clusters(self._h, _p(lo_a), _p(dims_a), self._cluster_flags(frontier, occ, infl, unknown), int(connectivity),
                                              int(min_size), *ptr, int(cap), None if sm is None else _p(sm)), "mlm_export_clusters")
        return sm

    @staticmethod
    def _cluster_flags(frontier, occ, infl, unknown) -> int:
        return ((MLM_CLUSTER_FRONTIER if frontier else 0) | (MLM_CLUSTER_OCC if occ else 0) | (MLM_CLUSTER_INFL if infl else 0) |
                (MLM_CLUSTER_UNKNOWN if unknown else 0))

    def export_mesh(self, lo, dims, occ=True, infl=False, unknown=False, seen=False, closed=False, normals=True) -> Dict[str, np.ndarray]:
        """Exact surface mesh of the obstacle set (the union of occ / infl / unknown as in export_esdf) of the box lo <= v < lo + dims
        (voxel indices as export_window): the voxel faces between an obstacle and an open voxel, as quads over shared vertices.
        seen: only faces towards FREE voxels; closed: everything outside the box counts as open, the mesh is the closed boundary of
        the box's obstacles.  Sizes the arrays with a summary-only call, then fills them: {"quads": int32 (F, 4) vertex numbers,
        counter-clockwise seen from outside (triangles: 0 1 2 and 0 2 3); "faces": int32 (F, 4) voxel x y z and direction 0..5 (-x +x
        -y +y -z +z); "verts": int32 (V, 3) lattice coordinates; "xyz": float32 (V, 3) positions; "normals": int8 (V, 3) sums of
        the adjacent faces' normals (normals=True); "summary": int64 [F, V, obstacle voxels, those with a face, faces per direction x 6,
        faces at the box's rim, 0]} (mlm_export_mesh)."""
        lo_a, dims_a = self._window_args(lo, dims)
        flags = self._mesh_flags(occ, infl, unknown, seen, closed)
        sm = np.zeros(MLM_MESH_ROW, dtype=np.int64)
        self._chk(self._L.mlm_export_mesh(self._h, _p(lo_a), _p(dims_a), flags, None, None, 0, None, None, None, 0, _p(sm)), "mlm_export_mesh")
        F, V = int(sm[0]), int(sm[1])
        out = {"quads": np.empty((F, 4), dtype=np.int32), "faces": np.empty((F, 4), dtype=np.int32), "verts": np.empty((V, 3), dtype=np.int32),
               "xyz": np.empty((V, 3), dtype=np.float32), "summary": sm}
        if normals:
            out["normals"] = np.empty((V, 3), dtype=np.int8)
        if F:  # (F > 0 iff V > 0; a cap of 0 goes with no array)
            self._chk(self._L.mlm_export_mesh(self._h, _p(lo_a), _p(dims_a), flags, _p(out["quads"]), _p(out["faces"]), F, _p(out["verts"]),
                                              _p(out["xyz"]), _p(out["normals"]) if normals else None, V, _p(sm)), "mlm_export_mesh")
            if (int(sm[0]), int(sm[1])) != (F, V):
                raise MlmError("mlm_export_mesh: the map changed between the sizing call and the export")
        return out

    def export_mesh_dev(self, lo, dims, occ=True, infl=False, unknown=False, seen=False, closed=False, quads: Optional[int] = None,
                        faces: Optional[int] = None, cap_faces: int = 0, verts: Optional[int] = None, xyz: Optional[int] = None,
                        normals: Optional[int] = None, cap_verts: int = 0, summary: bool = True) -> Optional[np.ndarray]:
        """Same on device memory: quads / faces pointers (int) to cap_faces x 4 int32, verts to cap_verts x 3 int32, xyz to cap_verts x 3
        float32, normals to cap_verts x 3 int8, None = skipped (a cap is 0 iff all of its arrays are None); rows beyond a cap are
        not written.  summary=True returns the twelve int64 counters, which tell F and V whatever the caps."""
        lo_a, dims_a = self._window_args(lo, dims)
        sm = np.zeros(MLM_MESH_ROW, dtype=np.int64) if summary else None
        ptr = [None if v is None else ctypes.c_void_p(v) for v in (quads, faces, verts, xyz, normals)]
        self._chk(self._L.mlm_export_mesh(self._h, _p(lo_a), _p(dims_a), self._mesh_flags(occ, infl, unknown, seen, closed), ptr[0], ptr[1],
                                          int(cap_faces), ptr[2], ptr[3], ptr[4], int(cap_verts), None if sm is None else _p(sm)), "mlm_export_mesh")
        return sm

    @staticmethod
    def _mesh_flags(occ, infl, unknown, seen, closed) -> int:
        return ((MLM_MESH_OCC if occ else 0) | (MLM_MESH_INFL if infl else 0) | (MLM_MESH_UNKNOWN if unknown else 0) |
                (MLM_MESH_SEEN if seen else 0) | (MLM_MESH_CLOSED if closed else 0))

    def export_octree(self, lo=None, dims=None, depth: int = 16, infl=False, occ_only=False) -> Dict[str, np.ndarray]:
        """Exact pruned occupancy octree of the box lo <= v < lo + dims (voxel indices as export_window; no box: the bounding box of
        the block keys): a voxel is OCC if occ == OCCUPIED (infl: or infl == OCCUPIED), FREE if occ == FREE and not OCC (occ_only:
        never), NONE otherwise and outside the box; cells of the key lattice k = v + 2^(depth-1), level l = k >> l, eight equal
        leaves pruned into one.  Sizes the arrays with a summary-only call, then fills them: {"words": uint16 (N,) per inner node in
        depth-first pre-order the children's labels, child i at bits 2i (0 NONE, 1 FREE, 2 OCC, 3 INNER); "inner4": int32 (N, 4) lower
        corner x y z and level; "skip": int32 (N,) the next inner node outside the subtree; "leaf4": int32 (M, 4) lower corner and
        level, in Morton order; "leaf_class": int8 (M,) 0 OCCUPIED / 1 FREE; "summary": int64 [N, M, OCC leaves, FREE leaves, OCC
        voxels, FREE voxels, root label, 0, leaves per level x 32]; "lo", "dims": the box} (mlm_export_octree;
        mlmapping_amd.octree_io turns words into an OctoMap .bt stream)."""
        if lo is None or dims is None:
            keys = self.export_blocks()["keys"].astype(np.int64).reshape(-1, 3)
            if len(keys) == 0:
                lo, dims = (0, 0, 0), (1, 1, 1)
            else:
                lo = keys.min(axis=0) * self.cfg.subbox_n
                dims = (keys.max(axis=0) + 1) * self.cfg.subbox_n - lo
        lo_a, dims_a = self._window_args(lo, dims)
        flags = self._oct_flags(infl, occ_only)
        sm = np.zeros(MLM_OCT_ROW, dtype=np.int64)
        self._chk(self._L.mlm_export_octree(self._h, _p(lo_a), _p(dims_a), int(depth), flags, None, None, None, 0, None, None, 0, _p(sm)),
                  "mlm_export_octree")
        N, M = int(sm[0]), int(sm[1])
        out = {"words": np.empty(N, dtype=np.uint16), "inner4": np.empty((N, 4), dtype=np.int32), "skip": np.empty(N, dtype=np.int32),
               "leaf4": np.empty((M, 4), dtype=np.int32), "leaf_class": np.empty(M, dtype=np.int8), "summary": sm,
               "lo": lo_a.copy(), "dims": dims_a.copy()}
        if M:  # (N > 0 implies M > 0; a cap of 0 goes with no array)
            inner = [_p(out[k]) if N else None for k in ("words", "inner4", "skip")]
            self._chk(self._L.mlm_export_octree(self._h, _p(lo_a), _p(dims_a), int(depth), flags, *inner, N, _p(out["leaf4"]),
                                                _p(out["leaf_class"]), M, _p(sm)), "mlm_export_octree")
            if (int(sm[0]), int(sm[1])) != (N, M):
                raise MlmError("mlm_export_octree: the map changed between the sizing call and the export")
        return out

    def export_octree_dev(self, lo, dims, depth: int = 16, infl=False, occ_only=False, words: Optional[int] = None,
                          inner4: Optional[int] = None, skip: Optional[int] = None, cap_inner: int = 0, leaf4: Optional[int] = None,
                          leaf_class: Optional[int] = None, cap_leaves: int = 0, summary: bool = True) -> Optional[np.ndarray]:
        """Same on device memory: words a pointer (int) to cap_inner uint16, inner4 to cap_inner x 4 int32, skip to cap_inner int32,
        leaf4 to cap_leaves x 4 int32, leaf_class to cap_leaves int8, None = skipped (a cap is 0 iff all of its arrays are None); rows
        beyond a cap are not written.  summary=True returns the forty int64 counters, which tell N and M whatever the caps."""
        lo_a, dims_a = self._window_args(lo, dims)
        sm = np.zeros(MLM_OCT_ROW, dtype=np.int64) if summary else None
        ptr = [None if v is None else ctypes.c_void_p(v) for v in (words, inner4, skip, leaf4, leaf_class)]
        self._chk(self._L.mlm_export_octree(self._h, _p(lo_a), _p(dims_a), int(depth), self._oct_flags(infl, occ_only), ptr[0], ptr[1], ptr[2],
                                            int(cap_inner), ptr[3], ptr[4], int(cap_leaves), None if sm is None else _p(sm)), "mlm_export_octree")
        return sm

    @staticmethod
    def _oct_flags(infl, occ_only) -> int:
        return (MLM_OCT_INFL if infl else 0) | (MLM_OCT_OCC_ONLY if occ_only else 0)

    def cast_rays(self, p0, p1, occ=True, infl=False, unknown=False) -> Dict[str, np.ndarray]:
        """Cast the segments p0[i] -> p1[i] (n x 3 world positions) through the voxel map (mlm_query_rays): {"status": int8 (1
        stopped, 0 reached the end, -1 invalid ray), "voxel": int32 (n, 3) the stopping or the end voxel, "t": float64 segment
        parameter at which the stopping voxel is entered (1.0 without a stop), "n_steps": int32 path index of the stopping voxel
        (voxels visited without a stop), "n_unknown": int32 UNKNOWN voxels in front of it}.  A ray stops at the first voxel that is
        occ (getOccupancy == OCCUPIED), infl (getInflateOccupancy == OCCUPIED) or unknown (getOccupancy == UNKNOWN), whichever are
        selected; none selected: a pure count."""
        a, b = _f64(p0).reshape(-1, 3), _f64(p1).reshape(-1, 3)
        if a.shape != b.shape:
            raise MlmError("cast_rays: p0 and p1 differ in shape")
        n = a.shape[0]
        out = {"status": np.empty(n, dtype=np.int8), "voxel": np.empty((n, 3), dtype=np.int32), "t": np.empty(n, dtype=np.float64),
               "n_steps": np.empty(n, dtype=np.int32), "n_unknown": np.empty(n, dtype=np.int32)}
        self._chk(self._L.mlm_query_rays(self._h, _p(a), _p(b), n, self._ray_flags(occ, infl, unknown),
                                         *[_p(out[k]) for k in ("status", "voxel", "t", "n_steps", "n_unknown")]), "mlm_query_rays")
        return out

    def cast_rays_dev(self, p0: int, p1: int, n: int, occ=True, infl=False, unknown=False, status: Optional[int] = None,
                      voxel: Optional[int] = None, t: Optional[int] = None, n_steps: Optional[int] = None,
                      n_unknown: Optional[int] = None):
        """Same on device memory: pointers (ints) to n x 3 float64 end points and to n int8 / n x 3 int32 / n float64 / n int32 /
        n int32 outputs, None = skipped."""
        ptr = [None if v is None else ctypes.c_void_p(v) for v in (status, voxel, t, n_steps, n_unknown)]
        self._chk(self._L.mlm_query_rays(self._h, ctypes.c_void_p(p0), ctypes.c_void_p(p1), int(n),
                                         self._ray_flags(occ, infl, unknown), *ptr), "mlm_query_rays")

    def render_depth(self, T_ws=None, q_wb=None, t_wb=None, width: int = 0, height: int = 0, K=None, max_depth: float = 8.0, occ=True, infl=False,
                     unknown=False) -> Dict[str, np.ndarray]:
        """The depth images the map predicts for a pinhole camera (mlm_render_depth), one per pose.  Poses: T_ws (n, 12) float64 — R
        (3 x 3, sensor to world, row major) then the optical centre in the world — or q_wb (n, 4; w, x, y, z) and t_wb (n, 3), which
        compose_T_ws turns into T_ws with the configuration's T_bs (the poses update_map takes).  K = (fx, fy, cx, cy), None: the
        configuration's camera.  max_depth in metres (1 mm .. 65.535 m): where the pixels' rays end.  A ray stops as in cast_rays
        (occ / infl / unknown).  {"depth": uint16 (n, height, width) millimetres of z-depth as update_map reads them, 0 where
        nothing stopped the ray; "status": int8, "voxel": int32 (n, height, width, 3), "n_unknown": int32 as cast_rays' for the
        pixel's segment; "table": int64 (n, 4): stopped, not stopped, invalid pixels and the sum of n_unknown per pose}."""
        if T_ws is None:
            if q_wb is None or t_wb is None:
                raise MlmError("render_depth: give T_ws, or q_wb and t_wb")
            T = compose_T_ws(q_wb, t_wb, self.cfg.T_B_S)
        else:
            T = _f64(T_ws).reshape(-1, 12)
        n, w, hgt = T.shape[0], int(width), int(height)
        if w < 1 or hgt < 1:
            raise MlmError("render_depth: width and height must be >= 1")
        k = None if K is None else _f64(K).reshape(4)
        out = {"depth": np.empty((n, hgt, w), dtype=np.uint16), "status": np.empty((n, hgt, w), dtype=np.int8),
               "voxel": np.empty((n, hgt, w, 3), dtype=np.int32), "n_unknown": np.empty((n, hgt, w), dtype=np.int32),
               "table": np.empty((n, MLM_RENDER_ROW), dtype=np.int64)}
        self._chk(self._L.mlm_render_depth(self._h, _p(T), n, w, hgt, None if k is None else _p(k), self._depth_mm(max_depth),
                                           self._ray_flags(occ, infl, unknown), *[_p(out[c]) for c in ("depth", "status", "voxel", "n_unknown", "table")]),
                  "mlm_render_depth")
        return out

    def render_depth_dev(self, T_ws: int, n_poses: int, width: int, height: int, K=None, max_depth: float = 8.0, occ=True, infl=False,
                         unknown=False, depth: Optional[int] = None, status: Optional[int] = None, voxel: Optional[int] = None,
                         n_unknown: Optional[int] = None, table: Optional[int] = None):
        """Same on pointers (ints; device or host memory, each on its own): n_poses x 12 float64 poses, n_poses x height x width
        uint16 / int8 / 3 x int32 / int32 outputs, n_poses x 4 int64 table; None = skipped."""
        k = None if K is None else _f64(K).reshape(4)
        ptr = [None if v is None else ctypes.c_void_p(v) for v in (depth, status, voxel, n_unknown, table)]
        self._chk(self._L.mlm_render_depth(self._h, ctypes.c_void_p(T_ws), int(n_poses), int(width), int(height), None if k is None else _p(k),
                                           self._depth_mm(max_depth), self._ray_flags(occ, infl, unknown), *ptr), "mlm_render_depth")

    @staticmethod
    def _depth_mm(max_depth) -> int:
        mm = int(round(float(max_depth) * 1000.0))
        if not 1 <= mm <= 65535:
            raise MlmError("render_depth: max_depth must lie in 0.001 .. 65.535 m")
        return mm

    def query_views(self, p0, p1, view_begin, occ=True, infl=False, unknown=False, box=None, exclude=None, mark=False) -> Dict[str, np.ndarray]:
        """Distinct-voxel accounting of grouped ray fans (mlm_query_views): view k is the segments view_begin[k] .. view_begin[k + 1]
        of p0 / p1 (n x 3 world positions), walked as cast_rays walks them.  {"table": int64 (n_views, 8): distinct traversed
        voxels, of those UNKNOWN (the gain), of those FREE, distinct stop voxels, stopped rays, invalid rays, visits with
        multiplicity, refused; "mark": uint8 (dz, dy, dx) or absent}.  box = (lo, dims) restricts the accounting to a window (voxel
        indices as export_window); exclude: uint8 (dz, dy, dx), voxels with a non-zero byte are not counted; mark: True for a
        zeroed array, or a uint8 (dz, dy, dx) array that is updated in place (|= 1 traversed, |= 2 stop voxel) and returned."""
        a, b = _f64(p0).reshape(-1, 3), _f64(p1).reshape(-1, 3)
        vb = np.ascontiguousarray(view_begin, dtype=np.int32).reshape(-1)
        if a.shape != b.shape or vb.size < 1 or (vb.size > 1 and int(vb[-1]) > a.shape[0]):
            raise MlmError("query_views: p0 and p1 differ in shape, or view_begin is empty or reaches past the rays")
        lo_p = dims_p = ex_p = mk_p = None
        out = {"table": np.zeros((vb.size - 1, MLM_VIEW_ROW), dtype=np.int64)}
        if box is not None:
            lo_a, dims_a = self._window_args(*box)
            lo_p, dims_p = _p(lo_a), _p(dims_a)
            shape = (int(dims_a[2]), int(dims_a[1]), int(dims_a[0]))
            if exclude is not None:
                ex = np.ascontiguousarray(exclude, dtype=np.uint8)
                if ex.shape != shape:
                    raise MlmError("query_views: exclude must have the box's shape (dz, dy, dx)")
                ex_p = _p(ex)
            if mark is not False and mark is not None:
                mk = np.zeros(shape, dtype=np.uint8) if mark is True else mark
                if not (isinstance(mk, np.ndarray) and mk.dtype == np.uint8 and mk.shape == shape and mk.flags["C_CONTIGUOUS"]):
                    raise MlmError("query_views: mark must be a contiguous uint8 array of the box's shape (dz, dy, dx)")
                out["mark"] = mk
                mk_p = _p(mk)
        elif exclude is not None or (mark is not False and mark is not None):
            raise MlmError("query_views: exclude and mark need a box")
        self._chk(self._L.mlm_query_views(self._h, _p(a), _p(b), _p(vb), vb.size - 1, self._ray_flags(occ, infl, unknown), lo_p, dims_p, ex_p,
                                          mk_p, _p(out["table"])), "mlm_query_views")
        return out

    def query_views_dev(self, p0: int, p1: int, view_begin: int, n_views: int, occ=True, infl=False, unknown=False, box=None,
                        exclude: Optional[int] = None, mark: Optional[int] = None, table: Optional[int] = None):
        """Same on pointers (ints; device or host memory, each on its own): n x 3 float64 end points, n_views + 1 int32 view_begin,
        uint8 exclude / mark of the box, int64 n_views x 8 table; None = skipped."""
        lo_p = dims_p = None
        if box is not None:
            lo_a, dims_a = self._window_args(*box)
            lo_p, dims_p = _p(lo_a), _p(dims_a)
        ptr = [None if v is None else ctypes.c_void_p(v) for v in (exclude, mark, table)]
        self._chk(self._L.mlm_query_views(self._h, ctypes.c_void_p(p0), ctypes.c_void_p(p1), ctypes.c_void_p(view_begin), int(n_views),
                                          self._ray_flags(occ, infl, unknown), lo_p, dims_p, *ptr), "mlm_query_views")

    def query_boxes(self, boxes, occ=True, infl=False, unknown=False, max_grow=None, window=None):
        """Class counts and free-space growth of axis-aligned voxel boxes (mlm_query_boxes).  boxes: n x 6 int32, lo then hi,
        inclusive voxel indices as export_window — a numpy array (numpy results) or a torch device tensor (torch device results).
        A box is blocked by voxels that are occ (getOccupancy == OCCUPIED), infl (getInflateOccupancy == OCCUPIED) or unknown
        (getOccupancy == UNKNOWN), whichever are selected; none selected: nothing blocks.  max_grow: the most layers per face
        (-x, +x, -y, +y, -z, +z; one int for all six; None: a pure count of the boxes); window = (lo, dims): the box never leaves it.
        {"status": int8 (1 grown, 0 the box itself is blocked, -1 invalid), "box": int32 (n, 6) the final box, "closed": uint8, bit c
        set iff face c was closed by an obstacle (clear: by a limit), "table": int64 (n, 4): voxels of the final box, of those
        UNKNOWN, of those blocking (only at status 0), slabs absorbed}."""
        mg_p = lo_p = dims_p = None
        if max_grow is not None:
            mg = np.ascontiguousarray(np.broadcast_to(np.asarray(max_grow, dtype=np.int64), (6,)))
            if ((mg < -2 ** 31) | (mg >= 2 ** 31)).any():
                raise MlmError("query_boxes: max_grow does not fit an int32")
            mg = mg.astype(np.int32)
            mg_p = _p(mg)
        if window is not None:
            lo_a, dims_a = self._window_args(*window)
            lo_p, dims_p = _p(lo_a), _p(dims_a)
        flags = self._ray_flags(occ, infl, unknown)
        if isinstance(boxes, np.ndarray) or not hasattr(boxes, "data_ptr"):
            b = np.ascontiguousarray(np.asarray(boxes, dtype=np.int32).reshape(-1, 6))
            n = b.shape[0]
            out = {"status": np.empty(n, dtype=np.int8), "box": np.empty((n, 6), dtype=np.int32), "closed": np.empty(n, dtype=np.uint8),
                   "table": np.empty((n, MLM_BOX_ROW), dtype=np.int64)}
            ptr = [_p(b)] + [_p(out[k]) for k in ("status", "box", "closed", "table")]
        else:
            import torch

            if boxes.dtype != torch.int32 or boxes.numel() % 6 or not boxes.is_contiguous():
                raise MlmError("query_boxes: a tensor of boxes must be contiguous int32 with 6 words per box")
            n = boxes.numel() // 6
            dev = boxes.device
            out = {"status": torch.empty(n, dtype=torch.int8, device=dev), "box": torch.empty((n, 6), dtype=torch.int32, device=dev),
                   "closed": torch.empty(n, dtype=torch.uint8, device=dev), "table": torch.empty((n, MLM_BOX_ROW), dtype=torch.int64, device=dev)}
            ptr = [ctypes.c_void_p(boxes.data_ptr())] + [ctypes.c_void_p(out[k].data_ptr()) for k in ("status", "box", "closed", "table")]
        self._chk(self._L.mlm_query_boxes(self._h, ptr[0], n, flags, mg_p, lo_p, dims_p, *ptr[1:]), "mlm_query_boxes")
        return out

    def query_boxes_dev(self, boxes: int, n: int, occ=True, infl=False, unknown=False, max_grow=None, window=None,
                        status: Optional[int] = None, box: Optional[int] = None, closed: Optional[int] = None, table: Optional[int] = None):
        """Same on pointers (ints; device or host memory, each on its own): n x 6 int32 boxes, n int8 / n x 6 int32 / n uint8 /
        n x 4 int64 outputs, None = skipped."""
        mg_p = lo_p = dims_p = None
        if max_grow is not None:
            mg = np.ascontiguousarray(np.broadcast_to(np.asarray(max_grow, dtype=np.int32), (6,)))
            mg_p = _p(mg)
        if window is not None:
            lo_a, dims_a = self._window_args(*window)
            lo_p, dims_p = _p(lo_a), _p(dims_a)
        ptr = [None if v is None else ctypes.c_void_p(v) for v in (status, box, closed, table)]
        self._chk(self._L.mlm_query_boxes(self._h, ctypes.c_void_p(boxes), int(n), self._ray_flags(occ, infl, unknown), mg_p, lo_p, dims_p, *ptr),
                  "mlm_query_boxes")

    NEAREST_OUTPUTS = ("status", "voxel", "delta", "sq", "dist")

    def query_nearest(self, pos, max_dist, occ=True, infl=False, unknown=False, outputs=None):
        """The exact nearest obstacle voxel of each position (mlm_query_nearest).  pos: n x 3 float64 world positions — a numpy array
        (numpy results) or a torch device tensor (torch device results).  max_dist: 1 .. 64 voxels, the radius of the ball that is
        searched.  An obstacle is a voxel that is occ (getOccupancy == OCCUPIED), infl (getInflateOccupancy == OCCUPIED) or unknown
        (getOccupancy == UNKNOWN), whichever are selected (at least one).  outputs: the names wanted (None: all five).
        {"status": int8 (1 found, 0 nothing in range, -1 invalid position), "voxel": int32 (n, 3) the obstacle voxel (the
        position's own without one), "delta": int32 (n, 3) the vector from the position to that voxel's centre in 1/1024 voxel,
        "sq": int64 its squared length (-1 without an obstacle), "dist": float64 its length in metres (-1.0 without one)}."""
        names = self.NEAREST_OUTPUTS if outputs is None else tuple(outputs)
        if not names or any(k not in self.NEAREST_OUTPUTS for k in names):
            raise MlmError("query_nearest: outputs must name at least one of " + ", ".join(self.NEAREST_OUTPUTS))
        flags = self._ray_flags(occ, infl, unknown)
        if isinstance(pos, np.ndarray) or not hasattr(pos, "data_ptr"):
            p = _f64(pos).reshape(-1, 3)
            n = p.shape[0]
            shapes = {"status": ((n,), np.int8), "voxel": ((n, 3), np.int32), "delta": ((n, 3), np.int32), "sq": ((n,), np.int64),
                      "dist": ((n,), np.float64)}
            out = {k: np.empty(*shapes[k]) for k in names}
            ptr = [_p(p)] + [_p(out[k]) if k in out else None for k in self.NEAREST_OUTPUTS]
        else:
            import torch

            if pos.dtype != torch.float64 or pos.numel() % 3 or not pos.is_contiguous():
                raise MlmError("query_nearest: a tensor of positions must be contiguous float64 with 3 values per position")
            n = pos.numel() // 3
            dev = pos.device
            shapes = {"status": ((n,), torch.int8), "voxel": ((n, 3), torch.int32), "delta": ((n, 3), torch.int32), "sq": ((n,), torch.int64),
                      "dist": ((n,), torch.float64)}
            out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in names}
            ptr = [ctypes.c_void_p(pos.data_ptr())] + [ctypes.c_void_p(out[k].data_ptr()) if k in out else None for k in self.NEAREST_OUTPUTS]
        self._chk(self._L.mlm_query_nearest(self._h, ptr[0], n, int(max_dist), flags, *ptr[1:]), "mlm_query_nearest")
        return out

    def query_nearest_dev(self, pos: int, n: int, max_dist: int, occ=True, infl=False, unknown=False, status: Optional[int] = None,
                          voxel: Optional[int] = None, delta: Optional[int] = None, sq: Optional[int] = None, dist: Optional[int] = None):
        """Same on pointers (ints; device or host memory, each on its own): n x 3 float64 positions, n int8 / n x 3 int32 /
        n x 3 int32 / n int64 / n float64 outputs, None = skipped."""
        ptr = [None if v is None else ctypes.c_void_p(v) for v in (status, voxel, delta, sq, dist)]
        self._chk(self._L.mlm_query_nearest(self._h, ctypes.c_void_p(pos), int(n), int(max_dist), self._ray_flags(occ, infl, unknown), *ptr),
                  "mlm_query_nearest")

    SWEEP_OUTPUTS = ("status", "voxel", "t", "n_steps", "n_unknown", "hit", "hit_sq")

    def query_sweeps(self, p0, p1, radius, occ=True, infl=False, unknown=False, outputs=None):
        """Segment casts for a ball of `radius` voxels (mlm_query_sweeps): segment i runs from p0[i] to p1[i] (n x 3 float64 world
        positions — numpy arrays give numpy results, torch device tensors torch device results) and stops at the first path voxel
        within `radius` (0 .. 16, integer squared index distance) of a voxel that is occ (getOccupancy == OCCUPIED), infl
        (getInflateOccupancy == OCCUPIED) or unknown (getOccupancy == UNKNOWN), whichever are selected — export_reach's BLOCKED at
        that clearance.  outputs: the names wanted (None: all seven).  {"status", "voxel", "t", "n_steps", "n_unknown": as
        cast_rays', the voxel being the ball's centre; "hit": int32 (n, 3) the obstacle voxel responsible (smallest distance, then z,
        y, x; the end voxel without a stop), "hit_sq": int32 its squared distance from "voxel" (-1 without a stop)}."""
        names = self.SWEEP_OUTPUTS if outputs is None else tuple(outputs)
        if not names or any(k not in self.SWEEP_OUTPUTS for k in names):
            raise MlmError("query_sweeps: outputs must name at least one of " + ", ".join(self.SWEEP_OUTPUTS))
        flags = self._ray_flags(occ, infl, unknown)
        if isinstance(p0, np.ndarray) or not hasattr(p0, "data_ptr"):
            a, b = _f64(p0).reshape(-1, 3), _f64(p1).reshape(-1, 3)
            if a.shape != b.shape:
                raise MlmError("query_sweeps: p0 and p1 differ in shape")
            n = a.shape[0]
            shapes = {"status": ((n,), np.int8), "voxel": ((n, 3), np.int32), "t": ((n,), np.float64), "n_steps": ((n,), np.int32),
                      "n_unknown": ((n,), np.int32), "hit": ((n, 3), np.int32), "hit_sq": ((n,), np.int32)}
            out = {k: np.empty(*shapes[k]) for k in names}
            ptr = [_p(a), _p(b)] + [_p(out[k]) if k in out else None for k in self.SWEEP_OUTPUTS]
        else:
            import torch

            for x in (p0, p1):
                if not hasattr(x, "data_ptr") or x.dtype != torch.float64 or x.numel() % 3 or not x.is_contiguous():
                    raise MlmError("query_sweeps: tensors of end points must be contiguous float64 with 3 values per point")
            if p0.numel() != p1.numel() or p0.device != p1.device:
                raise MlmError("query_sweeps: p0 and p1 differ in size or device")
            n = p0.numel() // 3
            dev = p0.device
            shapes = {"status": ((n,), torch.int8), "voxel": ((n, 3), torch.int32), "t": ((n,), torch.float64), "n_steps": ((n,), torch.int32),
                      "n_unknown": ((n,), torch.int32), "hit": ((n, 3), torch.int32), "hit_sq": ((n,), torch.int32)}
            out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in names}
            ptr = [ctypes.c_void_p(p0.data_ptr()), ctypes.c_void_p(p1.data_ptr())] + \
                  [ctypes.c_void_p(out[k].data_ptr()) if k in out else None for k in self.SWEEP_OUTPUTS]
        self._chk(self._L.mlm_query_sweeps(self._h, ptr[0], ptr[1], n, int(radius), flags, *ptr[2:]), "mlm_query_sweeps")
        return out

    PATH_OUTPUTS = ("status", "way", "length", "table")
    PATH_KINDS = {"reach": MLM_PATH_REACH, "route": MLM_PATH_ROUTE, MLM_PATH_REACH: MLM_PATH_REACH, MLM_PATH_ROUTE: MLM_PATH_ROUTE}

    @staticmethod
    def _path_max_moves(dims_a, max_moves) -> int:
        """None: eight times the box's edge sum, at most voxels - 1 (no genuine path is longer) and 2^20, at least 1"""
        if max_moves is not None:
            return int(max_moves)
        d = [int(v) for v in dims_a]
        return max(1, min(2 ** 20, d[0] * d[1] * d[2] - 1, 8 * sum(d)))

    def query_paths(self, lo, dims, parent, goals, kind="route", lookahead: int = 64, max_moves: Optional[int] = None, cap: int = 64,
                    outputs=None):
        """Paths through a parent field, traced and shortened to way points (mlm_query_paths).  lo, dims: the voxel box of the field
        (as export_window); parent: its uint8 bytes (dz, dy, dx) as export_route (kind "route") or export_reach (kind "reach") wrote
        them — a numpy array (the call runs on the host) or a torch device tensor (it runs as a kernel); goals: n x 3 int32 absolute
        voxel indices — a numpy array (numpy results) or a torch device tensor (torch device results).  lookahead: 1 .. 4096 moves,
        how far ahead of a way point the next one is looked for (1: the raw path); max_moves: 1 .. 2^20, the longest path traced
        (None: eight times the sum of the box's edges, at most the box's voxels - 1); cap: rows of "way" per goal.  outputs: the names
        wanted (None: all four).  {"status": int8 (1 path, 0 goal not reached or outside the box, -1 longer than max_moves, -2
        broken field), "way": int32 (n, cap, 3) the first min(W, cap) way points, goal first, seed last, zeros beyond, "length":
        float64 the way-point polyline in metres (-1.0 without a path), "table": int64 (n, 8) [moves K, way points W, face, edge,
        corner moves, longest leg in moves, candidates beyond the chosen ones, 0]}."""
        names = self.PATH_OUTPUTS if outputs is None else tuple(outputs)
        if not names or any(k not in self.PATH_OUTPUTS for k in names):
            raise MlmError("query_paths: outputs must name at least one of " + ", ".join(self.PATH_OUTPUTS))
        if kind not in self.PATH_KINDS:
            raise MlmError("query_paths: kind must be 'reach' or 'route'")
        lo_a, dims_a = self._window_args(lo, dims)
        nvox = int(dims_a[0]) * int(dims_a[1]) * int(dims_a[2])
        if isinstance(parent, np.ndarray) or not hasattr(parent, "data_ptr"):
            par = np.ascontiguousarray(np.asarray(parent, dtype=np.uint8))
            if par.size != nvox:
                raise MlmError("query_paths: parent must hold one byte per voxel of the box")
            par_p = _p(par)
        else:
            import torch

            if parent.dtype != torch.uint8 or parent.numel() != nvox or not parent.is_contiguous():
                raise MlmError("query_paths: a parent tensor must be contiguous uint8 with one byte per voxel of the box")
            par_p = ctypes.c_void_p(parent.data_ptr())
        cap = int(cap)
        if cap < 0 or (cap == 0 and "way" in names):
            raise MlmError("query_paths: cap must be >= 1 with the output 'way' (>= 0 without)")
        if "way" not in names:
            cap = 0
        if isinstance(goals, np.ndarray) or not hasattr(goals, "data_ptr"):
            g = np.ascontiguousarray(np.asarray(goals, dtype=np.int32).reshape(-1, 3))
            n = g.shape[0]
            shapes = {"status": ((n,), np.int8), "way": ((n, cap, 3), np.int32), "length": ((n,), np.float64),
                      "table": ((n, MLM_PATH_ROW), np.int64)}
            out = {k: np.zeros(*shapes[k]) for k in names}
            ptr = [_p(g)] + [_p(out[k]) if k in out else None for k in self.PATH_OUTPUTS]
        else:
            import torch

            if goals.dtype != torch.int32 or goals.numel() % 3 or not goals.is_contiguous():
                raise MlmError("query_paths: a tensor of goals must be contiguous int32 with 3 values per goal")
            n = goals.numel() // 3
            shapes = {"status": ((n,), torch.int8), "way": ((n, cap, 3), torch.int32), "length": ((n,), torch.float64),
                      "table": ((n, MLM_PATH_ROW), torch.int64)}
            out = {k: torch.zeros(shapes[k][0], dtype=shapes[k][1], device=goals.device) for k in names}
            ptr = [ctypes.c_void_p(goals.data_ptr())] + [ctypes.c_void_p(out[k].data_ptr()) if k in out else None for k in self.PATH_OUTPUTS]
        self._chk(self._L.mlm_query_paths(self._h, _p(lo_a), _p(dims_a), par_p, self.PATH_KINDS[kind], ptr[0], n, int(lookahead),
                                          self._path_max_moves(dims_a, max_moves), cap, *ptr[1:]), "mlm_query_paths")
        return out

    def query_paths_dev(self, lo, dims, parent: int, goals: int, n: int, kind="route", lookahead: int = 64, max_moves: Optional[int] = None,
                        cap: int = 0, status: Optional[int] = None, way: Optional[int] = None, length: Optional[int] = None,
                        table: Optional[int] = None):
        """Same on pointers (ints; device or host memory, each on its own): parent dz*dy*dx uint8, goals n x 3 int32, outputs n int8 /
        n x cap x 3 int32 / n float64 / n x 8 int64, None = skipped (cap 0 without way)."""
        if kind not in self.PATH_KINDS:
            raise MlmError("query_paths: kind must be 'reach' or 'route'")
        lo_a, dims_a = self._window_args(lo, dims)
        ptr = [None if v is None else ctypes.c_void_p(v) for v in (status, way, length, table)]
        self._chk(self._L.mlm_query_paths(self._h, _p(lo_a), _p(dims_a), ctypes.c_void_p(parent), self.PATH_KINDS[kind], ctypes.c_void_p(goals),
                                          int(n), int(lookahead), self._path_max_moves(dims_a, max_moves), int(cap), *ptr), "mlm_query_paths")

    def route_paths(self, lo, dims, seeds, goals, occ=True, infl=False, unknown=False, clearance: int = 0, connectivity: int = 26,
                    move_cost=(10, 14, 17), penalty=(), max_cost: Optional[int] = None, lookahead: int = 64,
                    max_moves: Optional[int] = None, cap: int = 64, outputs=None):
        """export_route into a device tensor, then query_paths on it: the way points from each goal to its cheapest seed; the field
        never leaves the device.  seeds: k x 3 voxel indices (array or int32 device tensor); goals and results as query_paths (plus
        "summary", export_route's four counters); the other arguments as export_route and query_paths."""
        import torch

        lo_a, dims_a = self._window_args(lo, dims)
        dev = torch.device("cuda", torch.cuda.current_device())
        if hasattr(seeds, "data_ptr"):
            if seeds.dtype != torch.int32 or seeds.numel() % 3 or not seeds.is_contiguous():
                raise MlmError("route_paths: a tensor of seeds must be contiguous int32 with 3 values per seed")
            s = seeds
        else:
            s = torch.from_numpy(np.ascontiguousarray(np.asarray(seeds, dtype=np.int32).reshape(-1, 3))).to(dev)
        field = torch.empty((int(dims_a[2]), int(dims_a[1]), int(dims_a[0])), dtype=torch.uint8, device=s.device)
        summary = self.export_route_dev(lo_a, dims_a, s.data_ptr(), s.numel() // 3, occ, infl, unknown, clearance, connectivity, move_cost,
                                        penalty, max_cost, parent=field.data_ptr(), summary=True)
        out = self.query_paths(lo_a, dims_a, field, goals, "route", lookahead, max_moves, cap, outputs)
        out["summary"] = summary
        return out

    SCORE_COLUMNS = ("valid", "occ", "free", "unknown", "infl", "in_box", "cost", "zero")

    def score_poses(self, pts_s, T_ws, classes=True, box=None, sqdist=None, sq_cap: int = 64):
        """Scan-to-map scores of candidate poses (mlm_score_poses).  pts_s: m x 3 float64 points in the sensor frame (backproject's,
        or any cloud), T_ws: n x 12 float64 poses as render_depth takes them (pose_grid's, compose_T_ws') — numpy arrays (numpy
        results) or torch device tensors (torch device results).  classes: count the classes of the voxels the points fall into.
        box = (lo, dims) and sqdist: a distance field over that voxel box, dz x dy x dx int32 as export_esdf's "sqdist" (a numpy
        array or a device tensor, whatever the rest is); the cost of a point is its sqdist clamped to 0 .. sq_cap, sq_cap outside
        the box.  Returns {"table": int64 (n, 8)} and its columns by name: "valid" pairs, those whose voxel is "occ", "free",
        "unknown" and "infl" (inflated-occupied), those "in_box", the summed "cost", and those in the box at sqdist <= 0 ("zero")."""
        if (box is None) != (sqdist is None):
            raise MlmError("score_poses: box and sqdist go together")
        on_dev = hasattr(pts_s, "data_ptr") and not isinstance(pts_s, np.ndarray)
        keep = []
        if on_dev:
            import torch

            for t, k, what in ((pts_s, 3, "points"), (T_ws, 12, "poses")):
                if not hasattr(t, "data_ptr") or t.dtype != torch.float64 or t.numel() % k or not t.is_contiguous():
                    raise MlmError(f"score_poses: a tensor of {what} must be contiguous float64 with {k} values per row")
            m, n = pts_s.numel() // 3, T_ws.numel() // 12
            table = torch.empty((n, MLM_SCORE_ROW), dtype=torch.int64, device=pts_s.device)
            ptr = [pts_s.data_ptr(), T_ws.data_ptr(), table.data_ptr()]
        else:
            p, T = _f64(pts_s).reshape(-1, 3), _f64(T_ws).reshape(-1, 12)
            keep += [p, T]
            m, n = p.shape[0], T.shape[0]
            table = np.empty((n, MLM_SCORE_ROW), dtype=np.int64)
            ptr = [p.ctypes.data, T.ctypes.data, table.ctypes.data]
        lo_a = dims_a = sq_p = None
        if box is not None:
            lo_a, dims_a = self._window_args(*box)
            nvox = int(dims_a[0]) * int(dims_a[1]) * int(dims_a[2])
            if hasattr(sqdist, "data_ptr") and not isinstance(sqdist, np.ndarray):
                import torch

                if sqdist.dtype != torch.int32 or sqdist.numel() != nvox or not sqdist.is_contiguous():
                    raise MlmError("score_poses: a tensor of sqdist must be contiguous int32 with one value per voxel of the box")
                sq_p = sqdist.data_ptr()
            else:
                f = np.ascontiguousarray(sqdist, dtype=np.int32)
                if f.size != nvox:
                    raise MlmError("score_poses: sqdist must hold one value per voxel of the box")
                keep.append(f)
                sq_p = f.ctypes.data
        self.score_poses_dev(ptr[0], m, ptr[1], n, ptr[2], classes, lo_a, dims_a, sq_p, sq_cap)
        out = {"table": table}
        for i, name in enumerate(self.SCORE_COLUMNS):
            out[name] = table[:, i]
        return out

    def score_poses_dev(self, pts_s: int, n_pts: int, T_ws: int, n_poses: int, table: int, classes=True, lo=None, dims=None,
                        sqdist: Optional[int] = None, sq_cap: int = 64):
        """Same on pointers (ints; device or host memory, each on its own): n_pts x 3 float64 points, n_poses x 12 float64 poses,
        n_poses x 8 int64 table; lo, dims and sqdist (dz*dy*dx int32) together or not at all."""
        lo_p = dims_p = None
        if lo is not None or dims is not None:
            lo_a, dims_a = self._window_args(lo, dims)
            lo_p, dims_p = _p(lo_a), _p(dims_a)
        vp = lambda v: None if v is None else ctypes.c_void_p(v)
        self._chk(self._L.mlm_score_poses(self._h, vp(pts_s), int(n_pts), vp(T_ws), int(n_poses), MLM_SCORE_CLASSES if classes else 0,
                                          lo_p, dims_p, vp(sqdist), int(sq_cap), vp(table)), "mlm_score_poses")

    CLEARANCE_OUTPUTS = ("status", "voxel", "t", "n_steps", "min_sq", "min", "cost", "n_near")

    def query_clearance(self, p0, p1, lo, dims, sqdist, sq_stop: int, sq_cap: int, outside_pass=False, group_begin=None, outputs=None):
        """Segment casts through a distance field (mlm_query_clearance): segment i runs from p0[i] to p1[i] (n x 3 float64 world
        positions — numpy arrays give numpy results, torch device tensors torch device results) along cast_rays' path through the
        field sqdist over the voxel box lo, dims (dz x dy x dx int32 as export_esdf's "sqdist"; a numpy array or a device tensor,
        whatever the rest is), f = sqdist clamped to 0 .. sq_cap.  The walk stops at the first path voxel with f <= sq_stop (status
        1; sq_stop -1: never) or outside the box (status 2; with outside_pass such voxels have f = sq_cap instead).  group_begin:
        n_groups + 1 int32 offsets into the segments (array or device tensor): one row per group in "table".  outputs: the names
        wanted (None: all eight; "table" comes with group_begin).  {"status": int8, "voxel": int32 (n, 3), "t": float64, "n_steps":
        int32, "min_sq": int32 the smallest f seen (-1: none), "min": int32 (n, 3) where, "cost": int64 the sum of sq_cap - f over
        the voxels passed, "n_near": int32 those with f < sq_cap, "table": int64 (n_groups, 8) [segments, first segment that did not
        reach its end or -1, its status, smallest min_sq up to it, which segment, summed cost, n_steps, n_near]}."""
        names = self.CLEARANCE_OUTPUTS if outputs is None else tuple(outputs)
        if any(k not in self.CLEARANCE_OUTPUTS for k in names) or (not names and group_begin is None):
            raise MlmError("query_clearance: outputs must name at least one of " + ", ".join(self.CLEARANCE_OUTPUTS) + " (or group_begin be given)")
        lo_a, dims_a = self._window_args(lo, dims)
        nvox = int(dims_a[0]) * int(dims_a[1]) * int(dims_a[2])
        keep = []
        if hasattr(sqdist, "data_ptr") and not isinstance(sqdist, np.ndarray):
            import torch

            if sqdist.dtype != torch.int32 or sqdist.numel() != nvox or not sqdist.is_contiguous():
                raise MlmError("query_clearance: a tensor of sqdist must be contiguous int32 with one value per voxel of the box")
            sq_p = ctypes.c_void_p(sqdist.data_ptr())
        else:
            f = np.ascontiguousarray(sqdist, dtype=np.int32)
            if f.size != nvox:
                raise MlmError("query_clearance: sqdist must hold one value per voxel of the box")
            keep.append(f)
            sq_p = _p(f)
        on_dev = hasattr(p0, "data_ptr") and not isinstance(p0, np.ndarray)
        if on_dev:
            import torch

            for x in (p0, p1):
                if not hasattr(x, "data_ptr") or x.dtype != torch.float64 or x.numel() % 3 or not x.is_contiguous():
                    raise MlmError("query_clearance: tensors of end points must be contiguous float64 with 3 values per point")
            if p0.numel() != p1.numel() or p0.device != p1.device:
                raise MlmError("query_clearance: p0 and p1 differ in size or device")
            n = p0.numel() // 3
            dev = p0.device
            shapes = {"status": ((n,), torch.int8), "voxel": ((n, 3), torch.int32), "t": ((n,), torch.float64), "n_steps": ((n,), torch.int32),
                      "min_sq": ((n,), torch.int32), "min": ((n, 3), torch.int32), "cost": ((n,), torch.int64), "n_near": ((n,), torch.int32)}
            out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in names}
            ptr = [ctypes.c_void_p(p0.data_ptr()), ctypes.c_void_p(p1.data_ptr())] + \
                  [ctypes.c_void_p(out[k].data_ptr()) if k in out else None for k in self.CLEARANCE_OUTPUTS]
        else:
            a, b = _f64(p0).reshape(-1, 3), _f64(p1).reshape(-1, 3)
            if a.shape != b.shape:
                raise MlmError("query_clearance: p0 and p1 differ in shape")
            n = a.shape[0]
            shapes = {"status": ((n,), np.int8), "voxel": ((n, 3), np.int32), "t": ((n,), np.float64), "n_steps": ((n,), np.int32),
                      "min_sq": ((n,), np.int32), "min": ((n, 3), np.int32), "cost": ((n,), np.int64), "n_near": ((n,), np.int32)}
            out = {k: np.empty(*shapes[k]) for k in names}
            ptr = [_p(a), _p(b)] + [_p(out[k]) if k in out else None for k in self.CLEARANCE_OUTPUTS]
        gb_p = tab_p = None
        ng = 0
        if group_begin is not None:
            if hasattr(group_begin, "data_ptr") and not isinstance(group_begin, np.ndarray):
                import torch

                if group_begin.dtype != torch.int32 or group_begin.numel() < 1 or not group_begin.is_contiguous():
                    raise MlmError("query_clearance: a tensor of group_begin must be contiguous int32 with at least one entry")
                ng = group_begin.numel() - 1
                gb_p = ctypes.c_void_p(group_begin.data_ptr())
            else:
                gb = np.ascontiguousarray(np.asarray(group_begin, dtype=np.int32).reshape(-1))
                if gb.size < 1:
                    raise MlmError("query_clearance: group_begin needs at least one entry")
                keep.append(gb)
                ng = gb.size - 1
                gb_p = _p(gb)
            if on_dev:
                out["table"] = torch.empty((ng, MLM_CLEAR_ROW), dtype=torch.int64, device=dev)
                tab_p = ctypes.c_void_p(out["table"].data_ptr())
            else:
                out["table"] = np.empty((ng, MLM_CLEAR_ROW), dtype=np.int64)
                tab_p = _p(out["table"])
        self._chk(self._L.mlm_query_clearance(self._h, ptr[0], ptr[1], n, _p(lo_a), _p(dims_a), sq_p, int(sq_stop), int(sq_cap),
                                              MLM_CLEAR_OUTSIDE_PASS if outside_pass else 0, *ptr[2:], gb_p, ng, tab_p), "mlm_query_clearance")
        return out

    def check_edges(self, p0, p1, radius: int, occ=True, infl=False, unknown=False, sq_cap: Optional[int] = None, group_begin=None,
                    max_voxels: int = 2 ** 28):
        """The edge check of a vehicle of `radius` voxels (0 .. 63) with its clearance along the edge: export_esdf {sqdist} over the
        voxel box of all end points into a device tensor, at max_dist = max(radius + 1, ceil(sqrt(sq_cap))) (at most 64; sq_cap None:
        (radius + 1)^2), then query_clearance on it with sq_stop = radius^2: the field never leaves the device.  A path never leaves
        the box of its two end voxels (every axis is monotone), so no walk leaves the box; status, voxel, t and n_steps are
        query_sweeps' at that radius.  p0, p1, group_begin and the results as query_clearance (numpy arrays are copied to the device
        and the results come back as numpy); occ, infl, unknown as export_esdf.  Raises ValueError, naming the box, when it holds
        more than max_voxels voxels: split the batch, or use query_sweeps, which needs no box."""
        import torch

        radius = int(radius)
        if radius < 0 or radius > 63:
            raise MlmError("check_edges: radius must lie in 0 .. 63")
        max_dist = radius + 1
        if sq_cap is None:
            sq_cap = max_dist * max_dist
        sq_cap = int(sq_cap)
        if sq_cap < 1 or sq_cap > 1 << 20:
            raise MlmError("check_edges: sq_cap must lie in 1 .. 2^20")
        root = math.isqrt(sq_cap)
        max_dist = min(64, max(max_dist, root if root * root == sq_cap else root + 1))
        host = not (hasattr(p0, "data_ptr") and not isinstance(p0, np.ndarray))
        dev = torch.device("cuda", torch.cuda.current_device())
        if host:
            a, b = _f64(p0).reshape(-1, 3), _f64(p1).reshape(-1, 3)
            if a.shape != b.shape:
                raise MlmError("check_edges: p0 and p1 differ in shape")
            p0, p1 = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        # the voxel box of the end points that lie on the lattice (the others belong to invalid segments)
        q = torch.floor((torch.cat([p0.reshape(-1, 3), p1.reshape(-1, 3)]) / self.cfg.subbox_d_xyz) * 1024.0)
        q = q[(q.abs() < 2.0 ** 40).all(dim=1)]
        if q.shape[0] == 0:
            lo_v, dims_v = [0, 0, 0], [1, 1, 1]
        else:
            v = torch.floor(q / 1024.0)
            vlo, vhi = v.min(dim=0).values.cpu().numpy().astype(np.int64), v.max(dim=0).values.cpu().numpy().astype(np.int64)
            lo_v, dims_v = [int(x) for x in vlo], [int(x) for x in vhi - vlo + 1]
        if dims_v[0] * dims_v[1] * dims_v[2] > int(max_voxels):
            raise ValueError(f"check_edges: the box of the end points, {dims_v[0]} x {dims_v[1]} x {dims_v[2]} voxels from {tuple(lo_v)}, holds more "
                             f"than max_voxels = {int(max_voxels)}: split the batch or use query_sweeps")
        lo_a, dims_a = self._window_args(lo_v, dims_v)
        field = torch.empty((dims_v[2], dims_v[1], dims_v[0]), dtype=torch.int32, device=p0.device)
        self.export_esdf_dev(lo_a, dims_a, max_dist, occ, infl, unknown, False, sqdist=field.data_ptr())
        if group_begin is not None and not (hasattr(group_begin, "data_ptr") and not isinstance(group_begin, np.ndarray)):
            group_begin = torch.from_numpy(np.ascontiguousarray(np.asarray(group_begin, dtype=np.int32).reshape(-1))).to(p0.device)
        out = self.query_clearance(p0, p1, lo_a, dims_a, field, radius * radius, sq_cap, False, group_begin)
        if host:
            out = {k: v.cpu().numpy() for k, v in out.items()}
        out["box"] = (np.asarray(lo_v, dtype=np.int64), np.asarray(dims_v, dtype=np.int64))
        return out

    def match_pose(self, pts_s, T_ws, lo, dims, max_dist: int = 8, occ=True, infl=False, unknown=False, classes=False):
        """export_esdf {sqdist} into a device tensor, then score_poses on it with sq_cap = max_dist^2: the likelihood-field cost of
        every candidate pose; the field never leaves the device.  pts_s, T_ws and the results as score_poses (numpy arrays are
        copied to the device and the table comes back as numpy); lo, dims, max_dist, occ, infl, unknown as export_esdf.  Adds
        "best": the index of the smallest cost, ties to the largest "occ", then to the lowest index."""
        import torch

        lo_a, dims_a = self._window_args(lo, dims)
        host = not (hasattr(pts_s, "data_ptr") and not isinstance(pts_s, np.ndarray))
        dev = torch.device("cuda", torch.cuda.current_device())
        if host:
            pts_s = torch.from_numpy(_f64(pts_s).reshape(-1, 3)).to(dev)
            T_ws = torch.from_numpy(_f64(T_ws).reshape(-1, 12)).to(dev)
        field = torch.empty((int(dims_a[2]), int(dims_a[1]), int(dims_a[0])), dtype=torch.int32, device=pts_s.device)
        self.export_esdf_dev(lo_a, dims_a, max_dist, occ, infl, unknown, False, sqdist=field.data_ptr())
        out = self.score_poses(pts_s, T_ws, classes, (lo_a, dims_a), field, int(max_dist) ** 2)
        t = out["table"].cpu().numpy()
        if host:
            out = {"table": t, **{name: t[:, i] for i, name in enumerate(self.SCORE_COLUMNS)}}
        out["best"] = best_score_row(t)
        return out

    @staticmethod
    def _ray_flags(occ, infl, unknown) -> int:
        return (MLM_RAY_OCC if occ else 0) | (MLM_RAY_INFL if infl else 0) | (MLM_RAY_UNKNOWN if unknown else 0)

    @staticmethod
    def _esdf_flags(occ, infl, unknown, signed) -> int:
        return ((MLM_ESDF_OCC if occ else 0) | (MLM_ESDF_INFL if infl else 0) | (MLM_ESDF_UNKNOWN if unknown else 0)
                | (MLM_ESDF_SIGNED if signed else 0))

    @staticmethod
    def _window_args(lo, dims):
        lo_a, dims_a = np.asarray(lo, dtype=np.int64).reshape(3), np.asarray(dims, dtype=np.int64).reshape(3)
        if ((lo_a < -2 ** 31) | (lo_a >= 2 ** 31) | (dims_a < 1) | (dims_a >= 2 ** 31)).any():
            raise MlmError("export_window: lo and dims are int32, dims >= 1")
        return lo_a.astype(np.int32), dims_a.astype(np.int32)

    def export_block_keys_dev(self, keys_dev_ptr: int, cap: int) -> int:
        """Block keys straight into device memory ([cap,3] int32); returns the block count."""
        m = ctypes.c_int32()
        self._chk(self._L.mlm_export_blocks(self._h, cap, ctypes.c_void_p(keys_dev_ptr), None, None, None, ctypes.byref(m)),
                  "mlm_export_blocks")
        return m.value

    def merge_pack(self, keys_dev_ptr: int, n: int, log_odds_dev_ptr: int, seen_dev_ptr: int):
        self._chk(self._L.mlm_merge_pack(self._h, ctypes.c_void_p(keys_dev_ptr), n, ctypes.c_void_p(log_odds_dev_ptr),
                                         ctypes.c_void_p(seen_dev_ptr)), "mlm_merge_pack")

    def merge_finish(self, log_odds_dev_ptr: int, seen_dev_ptr: int, n_cells: int, occ_dev_ptr: int):
        self._chk(self._L.mlm_merge_finish(self._h, ctypes.c_void_p(log_odds_dev_ptr), ctypes.c_void_p(seen_dev_ptr), n_cells,
                                           ctypes.c_void_p(occ_dev_ptr)), "mlm_merge_finish")

    def class_counts(self) -> Dict[str, int]:
        b = self.export_blocks()
        return {"blocks": int(b["keys"].shape[0]), "o": int((b["occ"] == ord("o")).sum()),
                "f": int((b["occ"] == ord("f")).sum())}

    def global_map_points(self) -> np.ndarray:
        """float32 [n,3] centres of the inflated-'o' cells: the PointCloud2 payload of /global_map."""
        n = ctypes.c_int32()
        self._chk(self._L.mlm_export_global_map(self._h, 0, None, ctypes.byref(n)), "mlm_export_global_map")
        out = np.empty((n.value, 3), dtype=np.float32)
        if n.value:
            self._chk(self._L.mlm_export_global_map(self._h, n.value, _p(out), ctypes.byref(n)), "mlm_export_global_map")
        return out

    def awareness_hits(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(cell idx sorted, odds, first-touch time) of the last frame."""
        n = self.frame_stats()["n_hit_cells"]
        cell = np.empty(n, dtype=np.uint32)
        odds = np.empty(n, dtype=np.float32)
        t = np.empty(n, dtype=np.uint32)
        m = ctypes.c_int32()
        self._chk(self._L.mlm_get_awareness_hits(self._h, n, _p(cell), _p(odds), _p(t), ctypes.byref(m)),
                  "mlm_get_awareness_hits")
        o = np.argsort(cell, kind="stable")
        return cell[o].astype(np.int64), odds[o], t[o]

    def awareness_misses(self) -> np.ndarray:
        n = self.frame_stats()["n_miss_cells"]
        cell = np.empty(n, dtype=np.uint32)
        m = ctypes.c_int32()
        self._chk(self._L.mlm_get_awareness_misses(self._h, n, _p(cell), ctypes.byref(m)), "mlm_get_awareness_misses")
        return np.sort(cell).astype(np.int64)

    def T_ls(self):
        q, t = np.empty(4), np.empty(3)
        self._chk(self._L.mlm_get_T_ls(self._h, _p(q), _p(t)), "mlm_get_T_ls")
        return q, t

    def odds_table(self) -> np.ndarray:
        out = np.empty((21, self.cfg.am_n_Rho), dtype=np.float32)
        self._chk(self._L.mlm_get_odds_table(self._h, _p(out)), "mlm_get_odds_table")
        return out

    def enable_kernel_timing(self, on=True):
        """True/1: per call; 2: accumulate over calls until kernel_times() is read; False/0: off."""
        self._chk(self._L.mlm_enable_kernel_timing(self._h, int(on)), "mlm_enable_kernel_timing")

    def set_timed_kernel(self, name: str, every: int = 1):
        """The one kernel whose launches (every `every`-th of them) timing mode 3 brackets."""
        self._chk(self._L.mlm_set_timed_kernel(self._h, name.encode(), int(every)), "mlm_set_timed_kernel")

    def kernel_times(self, cap: int = 1 << 16) -> List[Tuple[str, float]]:
        names = (ctypes.c_char_p * cap)()
        ms = np.empty(cap, dtype=np.float32)
        n = ctypes.c_int32()
        self._chk(self._L.mlm_get_kernel_times(self._h, cap, names, _p(ms), ctypes.byref(n)), "mlm_get_kernel_times")
        return [(names[i].decode(), float(ms[i])) for i in range(min(n.value, cap))]


def pinhole_fan(width: int, height: int, fx: float, fy: float, cx: float, cy: float, max_range: float) -> np.ndarray:
    """The ray grid of a pinhole camera for query_views: (height * width, 3) float64 end points in the camera frame (x right, y down,
    z forward), one per pixel centre (u + 0.5, v + 0.5), each at distance max_range from the optical centre along its pixel's
    ray.  A convenience: nothing of it is part of mlm_query_views' contract, which starts at the end points it is given."""
    u, v = np.meshgrid(np.arange(width, dtype=np.float64) + 0.5, np.arange(height, dtype=np.float64) + 0.5)
    dirs = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1).reshape(-1, 3)
    return dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * float(max_range)


def fan_views(origins, rotations, fan):
    """(p0, p1, view_begin) of one view per pose for query_views: view k casts the end points `fan` (m x 3, sensor frame, e.g.
    pinhole_fan's) from origins[k] (world) turned by rotations[k] (3 x 3, sensor to world).  A convenience like pinhole_fan."""
    o = _f64(origins).reshape(-1, 3)
    R = _f64(rotations).reshape(-1, 3, 3)
    f = _f64(fan).reshape(-1, 3)
    if len(o) != len(R):
        raise MlmError("fan_views: one rotation per origin")
    p1 = o[:, None, :] + np.einsum("kij,mj->kmi", R, f)
    p0 = np.broadcast_to(o[:, None, :], p1.shape)
    return (np.ascontiguousarray(p0).reshape(-1, 3), np.ascontiguousarray(p1).reshape(-1, 3),
            (np.arange(len(o) + 1, dtype=np.int64) * len(f)).astype(np.int32))


def compose_T_ws(q_wb, t_wb, T_bs) -> np.ndarray:
    """(n, 12) float64 poses for render_depth from body poses: q_wb (n, 4; w, x, y, z, normalised here), t_wb (n, 3) and the
    body-to-sensor transform T_bs (4 x 4, row major: MapConfig.T_B_S): per pose the rotation R_wb R_bs (row major) followed by the
    optical centre t_wb + R_wb t_bs.  Plain numpy and a convenience: mlm_render_depth's contract starts at R and o as given, and
    this is not the operation order of the integrate calls' quaternion composition (the two agree to rounding)."""
    q = _f64(q_wb).reshape(-1, 4)
    t = _f64(t_wb).reshape(-1, 3)
    if len(q) != len(t):
        raise MlmError("compose_T_ws: one translation per quaternion")
    B = _f64(T_bs).reshape(4, 4)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    out = np.empty((len(q), 12), dtype=np.float64)
    out[:, :9] = (R @ B[:3, :3]).reshape(-1, 9)
    out[:, 9:] = t + R @ B[:3, 3]
    return out


def invert_T(T) -> np.ndarray:
    """The inverse of a rigid transform T (12 float64: R row major, then o) in the same layout: R^T, then -R^T o, in float64."""
    T = _f64(T).reshape(12)
    Rt = T[:9].reshape(3, 3).T
    return np.ascontiguousarray(np.concatenate([Rt.reshape(9), -(Rt @ T[9:])]))


def best_score_row(table) -> int:
    """The row of a score_poses table a matcher takes: the smallest cost [6], ties to the largest occ count [1], then to the lowest
    index; -1 for an empty table."""
    t = np.asarray(table, dtype=np.int64).reshape(-1, MLM_SCORE_ROW)
    if not len(t):
        return -1
    return int(np.lexsort((np.arange(len(t)), -t[:, 1], t[:, 6]))[0])


def backproject(depth_u16, K, step: int = 1) -> np.ndarray:
    """The sensor-frame points update_map makes of a depth image (project_depth's arithmetic, mlmap.cpp:338-346): every `step`-th
    pixel of every `step`-th row, v outer and u fastest, raw 0 skipped; depth = raw * (1 / 1000.0), x = (float(u) - float(cx)) * depth
    / float(fx) — the subtraction in float32, the rest in float64 — y likewise, z = depth.  K = (fx, fy, cx, cy).  (m, 3) float64."""
    img = np.asarray(depth_u16)
    if img.ndim != 2 or img.dtype != np.uint16 or int(step) < 1:
        raise MlmError("backproject: a 2-D uint16 image and step >= 1")
    fx, fy, cx, cy = (np.float32(k) for k in np.asarray(K, dtype=np.float64).reshape(4))
    v, u = np.meshgrid(np.arange(0, img.shape[0], int(step)), np.arange(0, img.shape[1], int(step)), indexing="ij")
    raw = img[v, u]
    keepm = raw != 0
    u, v, raw = u[keepm], v[keepm], raw[keepm]
    depth = raw.astype(np.float64) * (1.0 / 1000.0)
    x = (u.astype(np.float32) - cx).astype(np.float64) * depth / np.float64(fx)
    y = (v.astype(np.float32) - cy).astype(np.float64) * depth / np.float64(fy)
    return np.ascontiguousarray(np.stack([x, y, depth], axis=1))


def pose_grid(T_ws, d: float, half_xyz=(3, 3, 1), yaw_deg=(-2, -1, 0, 1, 2)) -> np.ndarray:
    """A correlative search grid around one pose T_ws (12 float64: R row major, then o): for every yaw (outermost; degrees about the
    world z axis through the optical centre, R' = Rz(yaw) R in float64) the translations o + (ix, iy, iz) * d with |ix| <= half_xyz[0]
    and so on, z outer, x fastest — neighbouring rows differ by one voxel in x, which is what score_poses gathers fastest.
    (len(yaw_deg) * (2 hz + 1) * (2 hy + 1) * (2 hx + 1), 12) float64."""
    T = _f64(T_ws).reshape(12)
    R, o = T[:9].reshape(3, 3), T[9:]
    hx, hy, hz = (int(h) for h in half_xyz)
    iz, iy, ix = np.meshgrid(np.arange(-hz, hz + 1), np.arange(-hy, hy + 1), np.arange(-hx, hx + 1), indexing="ij")
    off = np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1).astype(np.float64) * float(d)
    out = np.empty((len(yaw_deg), len(off), 12), dtype=np.float64)
    for k, deg in enumerate(yaw_deg):
        a = np.deg2rad(np.float64(deg))
        Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        out[k, :, :9] = (Rz @ R).reshape(9)
        out[k, :, 9:] = o + off
    return out.reshape(-1, 12)
