"""Ground truth of mlm_render_depth (include/mlmap_hip.h) for tests/test_render_plan.py and tests/test_gpu_render.py: the segment of a
pixel and the depth of a walked segment in numpy float64, elementwise and in the order the contract states (numpy fuses nothing), and
whole images walked by tests/raywalk_ref.py over voxel classes that do not come from the code under test.  Nothing here calls it."""
import numpy as np

from tests import raywalk_ref as rw

RENDER_ROW = 4


def segments(T_ws, width, height, K, max_depth_mm):
    """(p0, p1), each (n_poses, height, width, 3) float64: p0 = o, p1[a] = ((R[a][0] xs + R[a][1] ys) + R[a][2] zs) + o[a] with
    xs = ((u - cx) Z) / fx, ys = ((v - cy) Z) / fy, zs = Z = max_depth_mm / 1000"""
    T = np.asarray(T_ws, dtype=np.float64).reshape(-1, 12)
    fx, fy, cx, cy = (np.float64(k) for k in K)
    Z = np.float64(max_depth_mm) / np.float64(1000.0)
    with np.errstate(all="ignore"):
        xs = ((np.arange(width, dtype=np.float64) - cx) * Z) / fx
        ys = ((np.arange(height, dtype=np.float64) - cy) * Z) / fy
        R, o = T[:, :9].reshape(-1, 3, 3), T[:, 9:]
        p1 = np.empty((len(T), height, width, 3), dtype=np.float64)
        for a in range(3):
            r0, r1, r2, oa = (x[:, None, None] for x in (R[:, a, 0], R[:, a, 1], R[:, a, 2], o[:, a]))
            p1[..., a] = ((r0 * xs[None, None, :] + r1 * ys[None, :, None]) + r2 * Z) + oa
    p0 = np.ascontiguousarray(np.broadcast_to(o[:, None, None, :], p1.shape))
    return p0, p1


def depth_mm(status, t, max_depth_mm):
    """uint16: min(65535, max(1, floor(t * max_depth_mm + 0.5))) where status == 1, else 0"""
    z = np.asarray(t, dtype=np.float64) * np.float64(max_depth_mm)
    r = np.clip(np.floor(z + 0.5), 1.0, 65535.0)
    return np.where(np.asarray(status) == 1, r, 0.0).astype(np.uint16)


def table(status, n_unknown):
    """int64 (n_poses, 4) from (n_poses, height, width) arrays: stopped, not stopped, invalid pixels, the sum of n_unknown"""
    st = np.asarray(status).reshape(len(status), -1)
    nu = np.asarray(n_unknown).reshape(len(status), -1).astype(np.int64)
    return np.stack([(st == 1).sum(1), (st == 0).sum(1), (st == -1).sum(1), nu.sum(1)], axis=1).astype(np.int64)


def from_rays(r, n_poses, height, width, max_depth_mm):
    """mlm_render_depth's outputs from mlm_query_rays' outputs (a dict of flat arrays) for the segments of segments()"""
    shp = (n_poses, height, width)
    out = {"status": r["status"].reshape(shp), "voxel": r["voxel"].reshape(shp + (3,)), "n_unknown": r["n_unknown"].reshape(shp),
           "depth": depth_mm(r["status"], r["t"], max_depth_mm).reshape(shp)}
    out["table"] = table(out["status"], out["n_unknown"])
    return out


def render_all(T_ws, width, height, K, max_depth_mm, d, classes, flag_sets=rw.FLAG_SETS):
    """{flags: {"status", "voxel", "t", "n_steps", "n_unknown" (flat, per pixel), "depth", "table"}}, p0, p1 (flat), ties per pixel"""
    p0, p1 = segments(T_ws, width, height, K, max_depth_mm)
    p0, p1 = p0.reshape(-1, 3), p1.reshape(-1, 3)
    res, ties = rw.cast_all(p0, p1, d, classes, flag_sets)
    n = len(np.asarray(T_ws).reshape(-1, 12))
    for f in flag_sets:
        r = res[f]
        r["depth"] = depth_mm(r["status"], r["t"], max_depth_mm)
        r["table"] = table(r["status"].reshape(n, -1), r["n_unknown"].reshape(n, -1))
    return res, p0, p1, ties
