"""Times the all-results item queries against the single-answer calls on the same items and bounds, in one run:
host clock around the synchronising C call, --warm warm-ups (the candidate buffer has grown), median / min / max of --reps calls.
  cd_points_within   the vertices of mi355_synth.cloth_pair(--quads) against that cloth, rmax = one quad edge, in mesh order;
                     beside it cd_closest_points on the same points and radius
  cd_cast_rays_all   the 256 x 256 pinhole camera of tests/test_rays_gpu.py::test_depth_frame over cloth_pair(100); beside it cd_cast_rays
Each list query four ways: count only (cap_rows = 0), the rows alone, rows + IDs + dist / t, rows + every value.  One JSON line a query."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "gpu-computing-course_amd", "pyhost"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, _p)

import mi355_synth as synth  # noqa: E402
import mi355cd  # noqa: E402
import ray_ref as rr  # noqa: E402  (the camera)

vp = lambda a: a.ctypes.data_as(C.c_void_p)


def _times(fn, reps, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3)}


def _rows_calls(cd, fn, items, struct, shapes, reps, warm):
    n, tested = C.c_uint64(0), C.c_uint64(0)
    rc = fn(cd._ctx, vp(items), items.shape[0], None, 0, C.byref(n), C.byref(tested), None)
    assert rc in (mi355cd.CD_OK, mi355cd.CD_OVERFLOW), rc
    total = n.value
    rows = np.empty((max(total, 1), 2), np.uint32)
    vals = [np.empty((max(total, 1),) + s, dt) for dt, s in shapes]
    full = struct(*(a.ctypes.data for a in vals))
    first = struct(vals[0].ctypes.data, vals[1].ctypes.data)               # IDs and dist / t only
    call = lambda r, cap, out: fn(cd._ctx, vp(items), items.shape[0], r, cap, C.byref(n), None, out)
    res = {"items": int(items.shape[0]), "rows": int(total), "tested": int(tested.value)}
    res["count_only"] = _times(lambda: call(None, 0, None), reps, warm)
    res["rows_only"] = _times(lambda: call(vp(rows), total, None), reps, warm)
    res["rows_ids_dist"] = _times(lambda: call(vp(rows), total, C.byref(first)), reps, warm)
    res["rows_all_values"] = _times(lambda: call(vp(rows), total, C.byref(full)), reps, warm)
    assert n.value == total
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--quads", type=int, default=500)
    a = ap.parse_args()

    v, i = synth.cloth_pair(a.quads)
    with mi355cd.CollisionDetector(v, i) as cd:
        cd.build_tree()
        p4 = mi355cd.pack_points(cd.verts, 2.88 / a.quads)
        nv = p4.shape[0]
        face, ids, dist, q, uv = np.empty(nv, np.uint32), np.empty(nv, np.uint32), np.empty(nv), np.empty((nv, 3)), np.empty((nv, 2))
        feat, side, info = np.empty(nv, np.uint8), np.empty(nv, np.uint8), mi355cd.CdPointInfo()
        single = _times(lambda: cd.lib.cd_closest_points(cd._ctx, vp(p4), nv, 0, vp(face), vp(ids), vp(dist), vp(q), vp(uv), vp(feat), vp(side), C.byref(info)), a.reps, a.warm)
        face_only = _times(lambda: cd.lib.cd_closest_points(cd._ctx, vp(p4), nv, 0, vp(face), None, None, None, None, None, None, C.byref(info)), a.reps, a.warm)
        res = _rows_calls(cd, cd.lib.cd_points_within, p4, mi355cd.CdPointRows,
                          [(np.uint32, ()), (np.float64, ()), (np.float64, (3,)), (np.float64, (2,)), (np.uint8, ()), (np.uint8, ())], a.reps, a.warm)
        res.update(query="cd_points_within", triangles=int(i.shape[0]), closest_points_all_outputs=single, closest_points_face_only=face_only,
                   closest_points_tri_tests=int(info.tri_tests))
        print(json.dumps(res), flush=True)

    v, i = synth.cloth_pair(100)
    rays = rr.pinhole(eye=[1.5, 2.5, 0.75], target=[1.5, -0.1, 0.75], up=[0.0, 0.0, 1.0], fov_deg=70.0, res=256)
    with mi355cd.CollisionDetector(v, i) as cd:
        cd.build_tree()
        nr = rays.shape[0]
        face, ids, t, uv, side = np.empty(nr, np.uint32), np.empty(nr, np.uint32), np.empty(nr), np.empty((nr, 2)), np.empty(nr, np.uint8)
        info = mi355cd.CdRayInfo()
        single = _times(lambda: cd.lib.cd_cast_rays(cd._ctx, vp(rays), nr, 0, vp(face), vp(ids), vp(t), vp(uv), vp(side), C.byref(info)), a.reps, a.warm)
        res = _rows_calls(cd, cd.lib.cd_cast_rays_all, rays, mi355cd.CdRayRows, [(np.uint32, ()), (np.float64, ()), (np.float64, (2,)), (np.uint8, ())], a.reps, a.warm)
        res.update(query="cd_cast_rays_all", triangles=int(i.shape[0]), cast_rays_all_outputs=single, cast_rays_tri_tests=int(info.tri_tests),
                   cast_rays_hits=int(info.n_hits))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
